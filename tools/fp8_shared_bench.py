"""Shared-prefix decode attention over the FP8 KV cache at the BASELINE configs[4] shape (profiles/fp8_shared_prefix.txt).
python tools/fp8_shared_bench.py [kernel] [engine] [gqa8]

kernel: B = 512 sequences behind one 512-token prompt (2 shared blocks of 256) + 94 own keys each, H = 16, KVH = 8, D = 128: device events around
replays of a hipGraph of 28 launches over 28 distinct layer caches (nothing re-read from the infinity cache), three alternating rounds of
  plain    nvr_paged_attn_decode_fp8 (every sequence reads the common keys itself)
  shared   nvr_paged_attn_decode_shared_fp8
  shared16 nvr_paged_attn_decode_shared over a 16-bit cache
engine: Qwen3-0.6B random-init, kv_cache_dtype = "fp8", 512 x (512 shared + 64 own) prompt tokens, hipGraph + launch-ahead, ms per decode step with
shared_prefix_min_seqs at its default and at -1, two alternating rounds.
gqa8: the kernel measurement at 8 query heads per kv head (profiles/fp8_gqa8_shared.txt): H = 64, KVH = 8, D in {128, 64}, 512 and 64 sequences behind 512 and
2048 shared keys + 94 own keys each; plain = the per-pair MFMA launch without tickets, which is what an engine with shared_prefix_min_seqs = -1 launches.
Further arguments narrow or widen the sweep: d128 | d64, b<sequences> .., p<shared blocks of 256 keys> .. (e.g. gqa8 b96 b128 b192 b256 b384 p2 p4 p8)."""
import ctypes as C, gc, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, nvr_import
nvr = nvr_import.load(); l = nvr.lib(); nvr.check(l.nvr_device_set(0))
what = sys.argv[1:] or ["kernel", "engine"]


def kernel_times(B=512, H=16, KVH=8, D=128, BS=256, P=2, own=94, L=28, replays=20, with16=True):
    st = C.c_void_p(); nvr.check(l.nvr_stream_create(C.byref(st)))
    rng = np.random.default_rng(3)
    NB, S = P + B, P * BS
    bt = np.concatenate([np.tile(np.arange(P, dtype=np.int32), (B, 1)), P + np.arange(B, dtype=np.int32)[:, None], -np.ones((B, 1), np.int32)], 1)
    ctx = np.full(B, S + own, np.int32)
    d_bt, d_ctx = nvr.DeviceBuffer.from_numpy(bt), nvr.DeviceBuffer.from_numpy(ctx)
    meta = nvr.AttnMetaC(); meta.is_prefill = 0; meta.context_lens = d_ctx.ptr; meta.block_tables = d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = bt.shape[1], B, S + own
    q = nvr.DeviceBuffer.from_numpy(rng.standard_normal((B, H * D)).astype(np.float16))
    out = nvr.DeviceBuffer(B * H * D * 2)
    ws = nvr.DeviceBuffer(l.nvr_paged_attn_workspace_bytes(B, H, D, S + own + BS))
    n = NB * BS * KVH * D
    h8 = (rng.integers(0, 0x48, n, dtype=np.uint8) | (rng.integers(0, 2, n, dtype=np.uint8) << 7))      # |value| < 4, no NaN code
    h16 = rng.standard_normal(n, dtype=np.float32).astype(np.float16) if with16 else None
    c8 = [(nvr.DeviceBuffer.from_numpy(h8), nvr.DeviceBuffer.from_numpy(h8)) for _ in range(L)]
    c16 = [(nvr.DeviceBuffer.from_numpy(h16), nvr.DeviceBuffer.from_numpy(h16)) for _ in range(L if with16 else 0)]
    scale = float(1 / np.sqrt(D))
    routes = {
        "plain": lambda i: l.nvr_paged_attn_decode_fp8(q.ptr, H * D, c8[i][0].ptr, c8[i][1].ptr, C.byref(meta), H, KVH, D, BS, scale, 1.0, 1.0, out.ptr, ws.ptr, None, st),
        "shared": lambda i: l.nvr_paged_attn_decode_shared_fp8(q.ptr, H * D, c8[i][0].ptr, c8[i][1].ptr, C.byref(meta), H, KVH, D, BS, scale, 1.0, 1.0, S, None, None, None,
                                                               out.ptr, ws.ptr, st),
        "shared16": lambda i: l.nvr_paged_attn_decode_shared(q.ptr, H * D, c16[i][0].ptr, c16[i][1].ptr, C.byref(meta), H, KVH, D, BS, scale, S, None, None, None,
                                                             out.ptr, ws.ptr, st),
    }
    if not with16:
        del routes["shared16"]
    graphs = {}
    for name, fn in routes.items():
        nvr.check(l.nvr_graph_capture_begin(st))
        for i in range(L):
            nvr.check(fn(i))
        g = C.c_void_p(); nvr.check(l.nvr_graph_capture_end(st, C.byref(g))); graphs[name] = g
        for _ in range(3):
            nvr.check(l.nvr_graph_launch(g, st))
    nvr.check(l.nvr_stream_synchronize(st))
    a, b = C.c_void_p(), C.c_void_p(); l.nvr_event_create(C.byref(a)); l.nvr_event_create(C.byref(b))
    for rnd in range(3):
        row = []
        for name, g in graphs.items():
            l.nvr_event_record(a, st)
            for _ in range(replays):
                nvr.check(l.nvr_graph_launch(g, st))
            l.nvr_event_record(b, st)
            ms = C.c_float(); nvr.check(l.nvr_event_elapsed_ms(a, b, C.byref(ms)))
            row.append(f"{name} {ms.value * 1e3 / (replays * L):.2f} us")
        print(f"round {rnd}: " + ", ".join(row) + " per layer", flush=True)


def engine_step_ms(min_seqs, nseq=512, steps=24):
    mc = nvr.ModelConfig("qwen3-0.6b")
    eng = nvr.LLMEngine(nvr.Config(max_num_seqs=nseq, max_num_batched_tokens=65536, max_model_len=1024, kvcache_block_size=256, num_kvcache_blocks=nseq * 2 + 16,
                                   async_decode=1, kv_cache_dtype="fp8", shared_prefix_min_seqs=min_seqs), mc)
    shared = nvr.synthetic_tokens(512, 2, 0, mc.c.vocab_size).tolist()
    for i in range(nseq):
        eng.add_request(shared + nvr.synthetic_tokens(64, 1, i, mc.c.vocab_size).tolist(), nvr.SamplingParams(temperature=0.0, max_tokens=steps + 12, ignore_eos=True))
    while eng.step()["is_prefill"]:
        pass
    for _ in range(4):
        eng.step()
    nvr.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        eng.step()
    nvr.synchronize(); dt = (time.perf_counter() - t0) / steps
    res = (dt * 1e3, eng.model_runner.last_shared_prefix_len())
    del eng
    gc.collect()
    return res


if "kernel" in what:
    kernel_times()
if "gqa8" in what:
    pick = lambda c, dflt: [int(w[1:]) for w in what if w[0] == c and w[1:].isdigit()] or dflt   # d128 | d64, b<sequences>.., p<shared blocks of 256>..
    for D in pick("d", [128, 64]):
        for B in pick("b", [512, 64]):
            for P in pick("p", [2, 8]):
                print(f"H=64 KVH=8 D={D}: {B} sequences behind {P * 256} shared keys + 94 own", flush=True)
                kernel_times(B=B, H=64, KVH=8, D=D, P=P, with16=False)
                gc.collect()
if "engine" in what:
    for rnd in range(2):
        print(f"round {rnd}: " + ", ".join("shared_prefix_min_seqs=%d: %.3f ms per step (shared length %d)" % ((ms,) + engine_step_ms(ms)) for ms in (0, -1)), flush=True)
