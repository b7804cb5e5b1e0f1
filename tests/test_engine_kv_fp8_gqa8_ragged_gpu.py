"""GPU tests (-m gpu) of FP8-KV engines with 8 query heads per kv head whose decode batches are ragged: the step takes the work-balanced MFMA attention launch
(attn_share_fp8_mfma_kernel; nvr_runner_last_decode_ragged), eager and hipGraph replay agree bit for bit, and the launch changes the logits only within the
attention tolerance against the per-pair launch (NVR_ATTN_SHARE=0 when the runner is created).  Flow: tests/test_engine_kv_fp8_ragged_gpu.py; the batch is
its own, above the runner's floor for 8 heads per kv head at head_dim 64 (14 units of 64 keys per CU: the smallest measured win)."""
import gc
import os

import numpy as np
import pytest

import nvr_import
from test_engine_kv_fp8_ragged_gpu import LOGIT_TOL, MODEL, NSEQ, VOCAB

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu

MODEL8 = {**MODEL, "num_attention_heads": 64, "num_key_value_heads": 8, "head_dim": 64, "max_position_embeddings": 4096}
ECFG = dict(max_num_seqs=NSEQ, max_num_batched_tokens=65536, max_model_len=3072, kvcache_block_size=256, num_kvcache_blocks=NSEQ * 12 + 4, kv_cache_dtype="fp8",
            recompute_cached_prefix=1)
# 24 sequences of 380..2850 tokens: 192 pairs, 3727 units of 64 keys over the 8 kv heads = 14.6 per CU of 256 — between the floor (14) and the step to two
# workgroups per CU (16), so the four decode steps keep one share count
PROMPTS = [nvr.synthetic_tokens(int(380 * 7.5 ** (i / (NSEQ - 1))), 1, i, VOCAB).tolist() for i in range(NSEQ)]


def run(share=None, **cfg):
    """prefill + 4 greedy decode steps: per step (is_prefill, tokens, logits, last_decode_ragged)"""
    nvr.check(nvr.lib().nvr_device_set(0))
    nvr.lib().nvr_seq_reset_id_counter()
    old = os.environ.pop("NVR_ATTN_SHARE", None)
    if share is not None:
        os.environ["NVR_ATTN_SHARE"] = share
    try:
        e = nvr.LLMEngine(nvr.Config(**{**ECFG, **cfg}), nvr.ModelConfig(**MODEL8))
    finally:
        os.environ.pop("NVR_ATTN_SHARE", None)
        if old is not None:
            os.environ["NVR_ATTN_SHARE"] = old
    for p in PROMPTS:
        e.add_request(p, nvr.SamplingParams(temperature=0.0, max_tokens=5, ignore_eos=True))
    out = []
    while not e.is_finished():
        rec = e.step()
        out.append((bool(rec["is_prefill"]), rec["tokens"], e.model_runner.logits(rec["num_seqs"]).copy(), e.model_runner.last_decode_ragged()))
    nvr.synchronize()
    del e
    gc.collect()
    return out


@pytest.fixture(scope="module")
def runs():
    return {"eager": run(enforce_eager=1), "graph": run(enforce_eager=0), "plain": run(share="0", enforce_eager=1)}


def test_fp8_gqa8_engine_takes_the_work_balanced_launch_for_ragged_batches(runs):
    for name in ("eager", "graph"):
        forms = [(pre, ragged) for pre, _, _, ragged in runs[name]]
        assert sum(not pre for pre, _ in forms) == 4 and all(ragged == (not pre) for pre, ragged in forms), (name, forms)
    assert not any(s[3] for s in runs["plain"])


def test_fp8_gqa8_engine_ragged_graph_replay_equals_eager(runs):
    assert len(runs["eager"]) == len(runs["graph"])
    for k, ((_, t1, l1, _), (_, t2, l2, _)) in enumerate(zip(runs["eager"], runs["graph"])):
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"


def test_fp8_gqa8_engine_ragged_first_decode_step_logits(runs):
    """the first decode step reads the same cache bytes and inputs on both launches; measured max |dlogit| (MI355X): see DESIGN 6c"""
    k = next(i for i, s in enumerate(runs["eager"]) if not s[0])
    assert k >= 1 and runs["eager"][k - 1][1] == runs["plain"][k - 1][1]                   # the step in front is the (identical) prefill
    l1, l2 = runs["eager"][k][2], runs["plain"][k][2]
    d = np.abs(l1 - l2).max()
    print(f"work-balanced vs per-pair fp8 decode at G = 8, first decode step: max |dlogit| {d:.3e} (max |logit| {np.abs(l2).max():.2f})")
    assert d < LOGIT_TOL
