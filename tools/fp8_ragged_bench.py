"""Ragged decode batches over the FP8 KV cache: the work-balanced attention launch against the per-pair launch (profiles/fp8_ragged.txt).
python tools/fp8_ragged_bench.py [rounds]

Qwen3-0.6B random-init, kv_cache_dtype = "fp8", hipGraph + launch-ahead; ms per decode step with NVR_ATTN_SHARE unset and = 0 when the runner is created
(0: the per-pair launch for every batch, the routing before attn_share_fp8_kernel), alternating rounds, for
  ragged32   32 sequences of 256..8192 keys (geometric)
  ragged64   64 sequences of 64..4096 keys (geometric)
  uniform36  36 sequences of 1024 keys (288 pairs on 256 CUs: the pair-count case of the launch rule, not a ragged batch)
and, per run, nvr_runner_last_decode_ragged of the timed steps."""
import gc, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvr_import
nvr = nvr_import.load(); l = nvr.lib(); nvr.check(l.nvr_device_set(0))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
WORKLOADS = {
    "ragged32": [int(256 * 32 ** (i / 31)) for i in range(32)],
    "ragged64": [int(64 * 64 ** (i / 63)) for i in range(64)],
    "uniform36": [1024] * 36,
}


def step_ms(lens, share, steps=96):
    if share is None: os.environ.pop("NVR_ATTN_SHARE", None)
    else: os.environ["NVR_ATTN_SHARE"] = share
    mc = nvr.ModelConfig("qwen3-0.6b")
    nblk = sum((n + steps + 16 + 255) // 256 for n in lens) + 8
    eng = nvr.LLMEngine(nvr.Config(max_num_seqs=len(lens), max_num_batched_tokens=max(65536, max(lens) + 1), max_model_len=max(lens) + 256, kvcache_block_size=256,
                                   num_kvcache_blocks=nblk, async_decode=1, kv_cache_dtype="fp8"), mc)
    os.environ.pop("NVR_ATTN_SHARE", None)
    for i, n in enumerate(lens):
        eng.add_request(nvr.synthetic_tokens(n, 1, i, mc.c.vocab_size).tolist(), nvr.SamplingParams(temperature=0.0, max_tokens=steps + 12, ignore_eos=True))
    while eng.step()["is_prefill"]:
        pass
    for _ in range(4):
        eng.step()
    nvr.synchronize(); t0 = time.perf_counter()
    ragged = set()
    for _ in range(steps):
        eng.step(); ragged.add(eng.model_runner.last_decode_ragged())
    nvr.synchronize(); dt = (time.perf_counter() - t0) / steps
    del eng
    gc.collect()
    return dt * 1e3, sorted(ragged)


for rnd in range(rounds):
    for name, lens in WORKLOADS.items():
        row = ["NVR_ATTN_SHARE %s: %.3f ms per step (ragged %s)" % ((s or "unset",) + step_ms(lens, s)) for s in (None, "0")]
        print(f"round {rnd} {name}: " + ", ".join(row), flush=True)
