"""GPU tests (-m gpu) of runners whose decode-sized steps stream FP8 (e4m3) projection weights (Config(decode_weight_dtype="fp8")): the whole runner holds
ONE set of weight values (the dequantised ones), eager == hipGraph replay, the byte stream against the 16-bit route over the same values, refusals."""
import gc

import numpy as np
import pytest

import nvr_import
from test_engine_kv_fp8_gpu import BS, ECFG, MODEL, PROMPTS, _run
from test_linear_fp8_gpu import quant_ref

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-2                                                 # two routes over identical data at |logit| <~ 4 (tests/test_engine_kv_fp8_shared_gpu.py)
PROJ = {"qkv": "self_attn.qkv_proj", "o": "self_attn.o_proj", "gate_up": "mlp.gate_up_proj", "down": "mlp.down_proj"}


def _runner(**cfg):
    nvr.check(nvr.lib().nvr_device_set(0))
    return nvr.ModelRunner(nvr.Config(**{**ECFG, **cfg}), nvr.ModelConfig(**MODEL))


def test_fp8_runner_holds_one_set_of_weights():
    r8, ra = _runner(decode_weight_dtype="fp8"), _runner()
    assert r8.decode_weight_dtype() == "fp8_e4m3" and ra.decode_weight_dtype() == "float16"
    for name in (f"layers.{l}.{p}" for l in range(2) for p in PROJ):
        w8, wa = r8.weight(name).astype(np.float64), ra.weight(name).astype(np.float64)
        sc, again = quant_ref(w8)
        assert np.array_equal(again, w8), f"{name}: not a fixed point of quantise -> dequantise"
        # round to nearest: at most half the e4m3 spacing at |w| / scale (2^-9 below 2^-6), times the row's scale
        half_step = 0.5 * sc[:, None] * 2.0 ** (np.maximum(np.floor(np.log2(np.maximum(np.abs(wa) / sc[:, None], 2.0 ** -20))), -6) - 3)
        assert (np.abs(w8 - wa) <= half_step).all(), f"{name}: further than half an e4m3 step from the 16-bit weight"


def test_fp8_weight_engine_graph_replay_equals_eager():
    eager = _run(decode_weight_dtype="fp8", enforce_eager=1)[0]
    graph, _, _, facts = _run(decode_weight_dtype="fp8", enforce_eager=0)
    assert facts[3] > 0                                          # steps were launched ahead (async_decode at its default)
    for k, ((t1, l1), (t2, l2)) in enumerate(zip(eager, graph)):
        assert t1 == t2 and np.array_equal(l1, l2), f"step {k}: tokens or logit bits of the eager and the graph-replaying engine differ"


def _drive(r, forced=None, steps=5):
    """the engine's loop by hand (schedule, execute, postprocess) so that the tokens can be forced: per step (tokens fed back, logits)"""
    nvr.lib().nvr_seq_reset_id_counter()
    sched = nvr.Scheduler(nvr.Config(**ECFG))
    seqs = [nvr.Sequence(p, nvr.SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True), BS) for p in PROMPTS]
    for s in seqs:
        sched.add_sequence(s)
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


@pytest.mark.parametrize("kv", ["auto", "fp8"])
def test_fp8_weight_stream_against_the_16bit_route_on_the_same_values(kv):
    """the fp8 runner's read-back weights loaded into an "auto" runner: the prefill step (57 rows) and the decode steps run the byte stream there and
    the 16-bit kernels here over identical values and tokens; measured max |dlogit| (MI355X): see DESIGN 6d"""
    r8, ra = _runner(decode_weight_dtype="fp8", kv_cache_dtype=kv), _runner(kv_cache_dtype=kv)
    for l in range(2):
        for p, hf in PROJ.items():
            ra.load_tensor(f"model.layers.{l}.{hf}.weight", r8.weight(f"layers.{l}.{p}"))
    if kv == "fp8":
        r8.set_kv_scales(0.5, 2.0); ra.set_kv_scales(0.5, 2.0)
    a = _drive(r8)
    b = _drive(ra, forced=[t for t, _ in a])
    d = max(np.abs(x[1] - y[1]).max() for x, y in zip(a, b))
    print(f"fp8 weight stream vs 16-bit route on the same values (kv {kv}): max |dlogit| {d:.3e} (max |logit| {max(np.abs(y[1]).max() for y in b):.2f})")
    assert d < LOGIT_TOL
    del r8, ra
    gc.collect()


def test_fp8_weight_refusals_and_validation():
    for cfg, model in ((dict(dtype="float32"), {}), ({}, dict(use_bias=1)), (dict(tensor_parallel_size=2), {})):
        with pytest.raises(nvr.NvrError) as ex:
            nvr.ModelRunner(nvr.Config(**{**ECFG, "decode_weight_dtype": "fp8", **cfg}), nvr.ModelConfig(**{**MODEL, **model}))
        assert ex.value.code == -10 and "decode_weight_dtype" in str(ex.value), str(ex.value)
    with pytest.raises(nvr.NvrError) as ex:
        nvr.Config(decode_weight_dtype="int4").validate()
    assert ex.value.code == -7 and "Unsupported decode_weight_dtype: int4" in str(ex.value)
