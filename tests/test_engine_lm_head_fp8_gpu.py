"""GPU tests (-m gpu) of runners whose LM head streams FP8 (e4m3) bytes for steps of <= 64 LM-head rows (Config(decode_weight_dtype="fp8_head")): one set
of head (and tied embedding) values, eager == hipGraph replay with the token the arg-max of the logits read back, the byte stream against the 16-bit head
kernels over the same values, the refusal."""
import gc

import numpy as np
import pytest

import nvr_import
from test_engine_kv_fp8_gpu import BS, ECFG, MODEL, PROMPTS, VOCAB, _run
from test_linear_fp8_gpu import quant_ref

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu


def _runner(model=None, **cfg):
    nvr.check(nvr.lib().nvr_device_set(0))
    return nvr.ModelRunner(nvr.Config(**{**ECFG, **cfg}), nvr.ModelConfig(**{**MODEL, **(model or {})}))


def test_fp8_head_dtype_strings():
    nvr.Config(decode_weight_dtype="fp8_head").validate()        # (-7 without the value)
    assert _runner(decode_weight_dtype="fp8_head").decode_weight_dtype() == "fp8_e4m3_head"


@pytest.mark.parametrize("tied", [False, True])
def test_fp8_head_runner_holds_one_set_of_head_values(tied):
    m = dict(tie_word_embeddings=tied)
    rh, r8, ra = (_runner(m, decode_weight_dtype=d) for d in ("fp8_head", "fp8", "auto"))
    wh, wa = rh.weight("lm_head").astype(np.float64), ra.weight("lm_head").astype(np.float64)
    sc, again = quant_ref(wh)
    assert np.array_equal(again, wh), "not a fixed point of quantise -> dequantise"
    # round to nearest: at most half the e4m3 spacing at |w| / scale (2^-9 below 2^-6), times the row's scale (test_fp8_runner_holds_one_set_of_weights)
    half_step = 0.5 * sc[:, None] * 2.0 ** (np.maximum(np.floor(np.log2(np.maximum(np.abs(wa) / sc[:, None], 2.0 ** -20))), -6) - 3)
    assert (np.abs(wh - wa) <= half_step).all(), "further than half an e4m3 step from the 16-bit head"
    assert np.array_equal(rh.weight("embed"), rh.weight("lm_head") if tied else ra.weight("embed"))
    assert np.array_equal(r8.weight("lm_head"), ra.weight("lm_head")) and np.array_equal(r8.weight("embed"), ra.weight("embed"))   # "fp8": untouched


def test_fp8_head_engine_graph_replay_equals_eager():
    eager = _run(decode_weight_dtype="fp8_head", enforce_eager=1)[0]
    graph, _, _, facts = _run(decode_weight_dtype="fp8_head", enforce_eager=0)
    assert facts[3] > 0                                          # steps were launched ahead (async_decode at its default)
    for k, ((t1, l1), (t2, l2)) in enumerate(zip(eager, graph)):
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"
        assert list(t2) == l2.argmax(1).tolist(), f"step {k}: a token is not the lowest-index arg-max of the logits read back"


def _drive(r, cfg, prompts, forced=None, steps=4):
    """the engine's loop by hand (schedule, execute, postprocess) so that the tokens can be forced: per step (tokens fed back, logits)"""
    nvr.lib().nvr_seq_reset_id_counter()
    sched = nvr.Scheduler(nvr.Config(**cfg))
    for p in prompts:
        sched.add_sequence(nvr.Sequence(p, nvr.SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True), BS))
    out = []
    for k in range(steps):
        batch, prefill = sched.schedule()
        r.execute_model(batch, prefill)
        logits = r.logits(len(batch)).copy()
        toks = forced[k] if forced else logits.argmax(1).tolist()
        sched.postprocess(batch, toks)
        out.append((toks, logits))
    nvr.synchronize()
    return out


@pytest.mark.parametrize("kv,nseq", [("auto", 3), ("fp8", 3), ("auto", 40)])
def test_fp8_head_against_the_16bit_head_on_the_same_values(kv, nseq):
    """the "fp8_head" runner's head read-back loaded into a "fp8" runner: identical layers and tokens, the byte stream there (3 rows: the resident form,
    40 rows: three column tiles, chunked) and lm_head / gemm_tiled_lm_head here over identical values: two f32 summation orders, the kernel test's bound"""
    cfg = {**ECFG, "max_num_seqs": 64, "max_num_batched_tokens": 1024, "num_kvcache_blocks": 128, "kv_cache_dtype": kv}
    prompts = PROMPTS if nseq == 3 else [nvr.synthetic_tokens(5 + i % 3, 1, i, VOCAB).tolist() for i in range(nseq)]
    rh, r8 = _runner(**{**cfg, "decode_weight_dtype": "fp8_head"}), _runner(**{**cfg, "decode_weight_dtype": "fp8"})
    r8.load_tensor("lm_head.weight", rh.weight("lm_head"))
    if kv == "fp8":
        rh.set_kv_scales(0.5, 2.0); r8.set_kv_scales(0.5, 2.0)
    a = _drive(rh, cfg, prompts)
    b = _drive(r8, cfg, prompts, forced=[t for t, _ in a])
    assert all(len(t) == nseq for t, _ in a)
    print(f"fp8 head vs 16-bit head on the same values (kv {kv}, {nseq} rows): max |dlogit| {max(np.abs(x[1] - y[1]).max() for x, y in zip(a, b)):.3e} "
          f"(max |logit| {max(np.abs(y[1]).max() for y in b):.2f})")
    for (_, la), (_, lb) in zip(a, b):
        np.testing.assert_allclose(la, lb, rtol=2e-5, atol=3e-4)
    del rh, r8
    gc.collect()


def test_fp8_head_refuses_a_vocabulary_that_is_no_multiple_of_16():
    with pytest.raises(nvr.NvrError) as ex:
        _runner(dict(vocab_size=VOCAB + 8), decode_weight_dtype="fp8_head")
    assert ex.value.code == -10 and "decode_weight_dtype" in str(ex.value), str(ex.value)
