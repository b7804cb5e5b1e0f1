"""Decode attention at 8 query heads per kv head: the FP8 KV cache on the matrix cores against the 16-bit cache (profiles/fp8_gqa8.txt).
python tools/fp8_gqa8_bench.py

B = 32 sequences of 1024 keys, D = 128, block size 256, fp16 build; H = 64, KVH = 8 (the Qwen3-32B heads on one GPU) and H = 8, KVH = 1 (a rank of 8).
Device events around replays of a hipGraph of 28 launches over 28 distinct layer caches (nothing re-read from the infinity cache), three alternating
rounds of
  fp8    nvr_paged_attn_decode_fp8   (attn_fp8_mfma_kernel, + the merge launch where the context is split)
  fp16   nvr_paged_attn_decode       (the 16-bit G = 8 launch of the same library: what these models run without the option)
TB/s is each kernel's own K + V bytes (B * ctx * KVH * D * 2 * element size) over its time."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, nvr_import
nvr = nvr_import.load(); l = nvr.lib(); nvr.check(l.nvr_device_set(0))


def kernel_times(H, KVH, B=32, D=128, BS=256, ctx_len=1024, L=28, replays=20):
    st = C.c_void_p(); nvr.check(l.nvr_stream_create(C.byref(st)))
    rng = np.random.default_rng(3)
    nb = ctx_len // BS
    NB = B * nb
    bt = np.concatenate([rng.permutation(NB).astype(np.int32).reshape(B, nb), -np.ones((B, 1), np.int32)], 1)
    d_bt, d_ctx = nvr.DeviceBuffer.from_numpy(bt), nvr.DeviceBuffer.from_numpy(np.full(B, ctx_len, np.int32))
    meta = nvr.AttnMetaC(); meta.is_prefill = 0; meta.context_lens = d_ctx.ptr; meta.block_tables = d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = bt.shape[1], B, ctx_len
    q = nvr.DeviceBuffer.from_numpy(rng.standard_normal((B, H * D)).astype(np.float16))
    out = nvr.DeviceBuffer(B * H * D * 2)
    ws = nvr.DeviceBuffer(l.nvr_paged_attn_workspace_bytes(B, H, D, ctx_len))
    n = NB * BS * KVH * D
    h8 = (rng.integers(0, 0x48, n, dtype=np.uint8) | (rng.integers(0, 2, n, dtype=np.uint8) << 7))      # |value| < 4, no NaN code
    h16 = rng.standard_normal(n, dtype=np.float32).astype(np.float16)
    c8 = [(nvr.DeviceBuffer.from_numpy(h8), nvr.DeviceBuffer.from_numpy(h8)) for _ in range(L)]
    c16 = [(nvr.DeviceBuffer.from_numpy(h16), nvr.DeviceBuffer.from_numpy(h16)) for _ in range(L)]
    scale = float(1 / np.sqrt(D))
    routes = {
        "fp8": lambda i: l.nvr_paged_attn_decode_fp8(q.ptr, H * D, c8[i][0].ptr, c8[i][1].ptr, C.byref(meta), H, KVH, D, BS, scale, 1.0, 1.0, out.ptr, ws.ptr, None, st),
        "fp16": lambda i: l.nvr_paged_attn_decode(q.ptr, H * D, c16[i][0].ptr, c16[i][1].ptr, C.byref(meta), H, KVH, D, BS, scale, out.ptr, ws.ptr, st),
    }
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
    kv_bytes = {"fp8": 2 * B * ctx_len * KVH * D, "fp16": 4 * B * ctx_len * KVH * D}
    for rnd in range(3):
        us = {}
        for name, g in graphs.items():
            l.nvr_event_record(a, st)
            for _ in range(replays):
                nvr.check(l.nvr_graph_launch(g, st))
            l.nvr_event_record(b, st)
            ms = C.c_float(); nvr.check(l.nvr_event_elapsed_ms(a, b, C.byref(ms)))
            us[name] = ms.value * 1e3 / (replays * L)
        print(f"H={H} KVH={KVH} round {rnd}: " + ", ".join(f"{k} {v:.2f} us per layer ({kv_bytes[k] / v * 1e-6:.2f} TB/s)" for k, v in us.items())
              + f", fp8 / fp16 = {us['fp8'] / us['fp16']:.2f}", flush=True)


kernel_times(64, 8)
kernel_times(8, 1)
