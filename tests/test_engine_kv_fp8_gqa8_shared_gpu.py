"""GPU tests (-m gpu) of FP8-KV engines at 8 query heads per kv head whose decode batches share a cached prefix: test_engine_kv_fp8_shared_gpu.py's
prompts and three tests on that head shape (the shared pass is taken, eager and hipGraph replay agree in bits, the logits move within the attention tolerance)."""
import gc

import numpy as np
import pytest

import nvr_import
from test_engine_kv_fp8_shared_gpu import ECFG, LOGIT_TOL, MODEL, PROMPTS

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu

MODEL8 = {**MODEL, "num_attention_heads": 8, "num_key_value_heads": 1, "head_dim": 64}


@pytest.fixture(scope="module")
def runs():
    def run(**cfg):                                                       # prefill + 8 greedy decode steps: per step (tokens, logits, (num_seqs, shared length, shared rows))
        nvr.check(nvr.lib().nvr_device_set(0))
        nvr.lib().nvr_seq_reset_id_counter()
        e = nvr.LLMEngine(nvr.Config(**{**ECFG, **cfg}), nvr.ModelConfig(**MODEL8))
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


def test_fp8_gqa8_engine_takes_the_shared_prefix_pass(runs):
    assert (7, 128, 6) in [s[2] for s in runs["eager"]] and (7, 128, 6) in [s[2] for s in runs["graph"]]
    assert all(s[2][1:] == (0, 0) for s in runs["plain"])


def test_fp8_gqa8_engine_shared_prefix_graph_replay_equals_eager(runs):
    for k, ((t1, l1, _), (t2, l2, _)) in enumerate(zip(runs["eager"], runs["graph"])):
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"


def test_fp8_gqa8_engine_shared_prefix_first_decode_step_logits(runs):
    """the first decode step reads the same cache bytes and inputs on both routes; measured max |dlogit| (MI355X): 0 — at this shape both
    routes cut the keys into the same 64-key steps on kernels with the same rounding points, and what differs (f32 summation order) rounds away"""
    k = next(i for i, s in enumerate(runs["eager"]) if s[2][1] > 0)
    (t1, l1, f1), (t2, l2, f2) = runs["eager"][k], runs["plain"][k]
    assert k >= 1 and runs["eager"][k - 1][2][1] == 0 and runs["eager"][k - 1][0] == runs["plain"][k - 1][0]   # the step in front is the (identical) prefill
    d = np.abs(l1 - l2).max()
    print(f"shared-prefix pass vs plain fp8 decode, first decode step: max |dlogit| {d:.3e} (max |logit| {np.abs(l2).max():.2f})")
    assert d < LOGIT_TOL
