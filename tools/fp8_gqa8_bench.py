"""Decode attention at 8 query heads per kv head: the FP8 KV cache on the matrix cores against the 16-bit cache (profiles/fp8_gqa8.txt).
python tools/fp8_gqa8_bench.py
python tools/fp8_gqa8_bench.py ragged      (the work-balanced launch against the per-pair one on ragged batches: ragged_times, profiles/fp8_gqa8_ragged.txt)

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


def ragged_times(name, lens, H=64, KVH=8, D=128, BS=256, replays=20):
    """python tools/fp8_gqa8_bench.py ragged (profiles/fp8_gqa8_ragged.txt): the work-balanced launch (attn_share_fp8_mfma_kernel: the call WITH tickets, where the
    launch rule takes it — NVR_ATTN_SHARE unset: the pair-count case, one workgroup per CU; = 2: every shape, two per CU) against the per-pair launch of the same
    library (no tickets: attn_fp8_mfma_kernel + merge), graphs over enough distinct layer caches to exceed the infinity cache, three alternating rounds."""
    st = C.c_void_p(); nvr.check(l.nvr_stream_create(C.byref(st)))
    rng = np.random.default_rng(3)
    B, nbs = len(lens), [(n + BS - 1) // BS for n in lens]
    NB, mb = sum(nbs), max(nbs) + 1
    bt, perm, o = -np.ones((B, mb), np.int32), rng.permutation(NB).astype(np.int32), 0
    for b, n in enumerate(nbs):
        bt[b, :n] = perm[o:o + n]; o += n
    d_bt, d_ctx = nvr.DeviceBuffer.from_numpy(bt), nvr.DeviceBuffer.from_numpy(np.asarray(lens, np.int32))
    meta = nvr.AttnMetaC(); meta.is_prefill = 0; meta.context_lens = d_ctx.ptr; meta.block_tables = d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = mb, B, max(lens)
    q = nvr.DeviceBuffer.from_numpy(rng.standard_normal((B, H * D)).astype(np.float16))
    out = nvr.DeviceBuffer(B * H * D * 2)
    ws = nvr.DeviceBuffer(l.nvr_paged_attn_workspace_bytes(B, H, D, max(lens)))
    tickets = nvr.DeviceBuffer.from_numpy(np.zeros(B * KVH, np.uint32))
    n = NB * BS * KVH * D
    L = max(4, -(-640_000_000 // (2 * n)))
    h8 = (rng.integers(0, 0x48, n, dtype=np.uint8) | (rng.integers(0, 2, n, dtype=np.uint8) << 7))      # |value| < 4, no NaN code
    c8 = [(nvr.DeviceBuffer.from_numpy(h8), nvr.DeviceBuffer.from_numpy(h8)) for _ in range(L)]
    scale = float(1 / np.sqrt(D))
    graphs = {}
    for route, tk in (("per-pair", None), ("balanced", tickets.ptr)):
        nvr.check(l.nvr_graph_capture_begin(st))
        for i in range(L):
            nvr.check(l.nvr_paged_attn_decode_fp8(q.ptr, H * D, c8[i][0].ptr, c8[i][1].ptr, C.byref(meta), H, KVH, D, BS, scale, 1.0, 1.0, out.ptr, ws.ptr, tk, st))
        g = C.c_void_p(); nvr.check(l.nvr_graph_capture_end(st, C.byref(g))); graphs[route] = g
        for _ in range(3):
            nvr.check(l.nvr_graph_launch(g, st))
    nvr.check(l.nvr_stream_synchronize(st))
    a, b = C.c_void_p(), C.c_void_p(); l.nvr_event_create(C.byref(a)); l.nvr_event_create(C.byref(b))
    for rnd in range(3):
        us = {}
        for route, g in graphs.items():
            l.nvr_event_record(a, st)
            for _ in range(replays):
                nvr.check(l.nvr_graph_launch(g, st))
            l.nvr_event_record(b, st)
            ms = C.c_float(); nvr.check(l.nvr_event_elapsed_ms(a, b, C.byref(ms)))
            us[route] = ms.value * 1e3 / (replays * L)
        print(f"NVR_ATTN_SHARE={os.environ.get('NVR_ATTN_SHARE', 'unset')} {name} ({B * KVH} pairs, {sum(-(-n // 64) for n in lens) * KVH} units, {L} layer caches) round {rnd}: "
              + ", ".join(f"{k} {v:.2f} us per layer ({2 * sum(lens) * KVH * D / v * 1e-6:.2f} TB/s)" for k, v in us.items())
              + f", balanced / per-pair = {us['balanced'] / us['per-pair']:.3f}", flush=True)


if sys.argv[1:] == ["ragged"]:
    ragged_times("ragged32", [int(256 * 32 ** (i / 31)) for i in range(32)])
    ragged_times("uniform36", [1024] * 36)
    ragged_times("ragged64", [int(64 * 64 ** (i / 63)) for i in range(64)])
    ragged_times("uniform32", [1024] * 32)
    for f in (1.0, 1.4, 1.8, 2.4):                                                  # 24 sequences of 200 f .. 1500 f keys: 7.6, 10.6, 13.7, 18.2 units of 64 keys per CU
        ragged_times(f"ragged24x{f}", [int(200 * f * 7.5 ** (i / 23)) for i in range(24)])
    ragged_times("ragged24x1.0 D=64", [int(200 * 7.5 ** (i / 23)) for i in range(24)], D=64)
    ragged_times("ragged24x1.8 D=64", [int(360 * 7.5 ** (i / 23)) for i in range(24)], D=64)
    ragged_times("ragged32h", [int(128 * 32 ** (i / 31)) for i in range(32)])       # half of ragged32: 18 units per CU
else:
    kernel_times(64, 8)
    kernel_times(8, 1)
