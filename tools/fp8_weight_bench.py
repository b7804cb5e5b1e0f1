"""FP8 (e4m3) weight stream of the decode GEMMs against the 16-bit tiled-copy launches at the Qwen3-8B shapes (profiles/fp8_decode_weights.txt).
python tools/fp8_weight_bench.py [kernel] [engine] [head] [head_engine]     (default: kernel engine; head / head_engine: profiles/fp8_lm_head.txt)

kernel: per shape and T = 1, 32, 64: device events around replays of a hipGraph of L launches over L DISTINCT weight buffers (L x bytes >= 768 MB, nothing
re-read from the infinity cache), three alternating rounds of
  fp8    nvr_linear_fp8 / nvr_linear_silu_mul_fp8 / nvr_linear_splitk_fp8 over nvr_weight_quantize_fp8 bytes
  tiled  nvr_linear_tiled / nvr_linear_silu_mul_tiled / nvr_linear_splitk_tiled over nvr_retile_weight copies (the default runner's decode launches)
engine: Qwen3-8B random-init, 32 sequences of 64 prompt tokens, hipGraph + launch-ahead, ms per decode step with decode_weight_dtype "auto" and "fp8",
two alternating rounds.
head: the LM head 151 936 x 1024 and x 4096 at T = 1, 32, 64, partials only (what a greedy step asks for), measured like kernel:
  fp8    nvr_lm_head_fp8 over nvr_weight_quantize_fp8 bytes
  16bit  nvr_lm_head_tiled over the nvr_retile_weight copy (T <= 32) / nvr_lm_head over the row-major matrix (T > 32: the 128x128 tiles)
head_engine: Qwen3-0.6B and Qwen3-8B at 1 and 32 sequences, decode_weight_dtype "fp8" and "fp8_head", two alternating rounds."""
import ctypes as C, gc, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvr_import
nvr = nvr_import.load(); l = nvr.lib(); nvr.check(l.nvr_device_set(0))
what = sys.argv[1:] or ["kernel", "engine"]
SHAPES = [("qkv   plain", 4096, 6144), ("gate_up silu", 4096, 12288), ("o     split-k", 4096, 4096), ("down  split-k", 12288, 4096)]


def kernel_times(name, K, N, replays=30):
    st = C.c_void_p(); nvr.check(l.nvr_stream_create(C.byref(st)))
    form = name.split()[1]
    rows = 2 * N if form == "silu" else N
    L = max(4, -(-(768 << 20) // (rows * K)))
    x, out = nvr.DeviceBuffer(64 * K * 2), nvr.DeviceBuffer(max(64 * N * 2, 4 * 64 * N * 4))
    nvr.check(l.nvr_fill_weight(x.ptr, 64, K, K, K, 0, 0, 3, 1e-5, None))
    W, Wt, Wq, Ws = [], [], [], []
    for i in range(L):
        w, t, q, s = nvr.DeviceBuffer(rows * K * 2), nvr.DeviceBuffer(rows * K * 2), nvr.DeviceBuffer(rows * K), nvr.DeviceBuffer(rows * 4)
        nvr.check(l.nvr_fill_weight(w.ptr, rows, K, K, K, 0, 0, 5 + i, 1e-6, None))
        nvr.check(l.nvr_retile_weight(w.ptr, t.ptr, rows, K, 0, 0, 0, 0, None))
        nvr.check(l.nvr_weight_quantize_fp8(w.ptr, rows, K, q.ptr, s.ptr, None, None))
        W.append(w); Wt.append(t); Wq.append(q); Ws.append(s)
    nvr.synchronize()
    a, b = C.c_void_p(), C.c_void_p(); l.nvr_event_create(C.byref(a)); l.nvr_event_create(C.byref(b))
    for T in (1, 32, 64):
        S = 4                                                                              # (both runners' slice count at these shapes)
        routes = {
            "plain": {"fp8": lambda i: l.nvr_linear_fp8(x.ptr, K, Wq[i].ptr, Ws[i].ptr, T, K, N, out.ptr, st),
                      "tiled": lambda i: l.nvr_linear_tiled(x.ptr, K, W[i].ptr, Wt[i].ptr, T, K, N, out.ptr, 0, st)},
            "silu": {"fp8": lambda i: l.nvr_linear_silu_mul_fp8(x.ptr, K, Wq[i].ptr, Ws[i].ptr, T, K, N, out.ptr, st),
                     "tiled": lambda i: l.nvr_linear_silu_mul_tiled(x.ptr, K, W[i].ptr, Wt[i].ptr, T, K, N, out.ptr, st)},
            "split-k": {"fp8": lambda i: l.nvr_linear_splitk_fp8(x.ptr, K, Wq[i].ptr, Ws[i].ptr, T, K, N, S, out.ptr, st),
                        "tiled": lambda i: l.nvr_linear_splitk_tiled(x.ptr, K, W[i].ptr, Wt[i].ptr, T, K, N, S, out.ptr, st)},
        }[form]
        graphs = {}
        for rn, fn in routes.items():
            nvr.check(fn(0)); nvr.check(l.nvr_stream_synchronize(st))                      # (first call outside the capture: LDS opt-ins)
            nvr.check(l.nvr_graph_capture_begin(st))
            for i in range(L):
                nvr.check(fn(i))
            g = C.c_void_p(); nvr.check(l.nvr_graph_capture_end(st, C.byref(g))); graphs[rn] = g
            for _ in range(2):
                nvr.check(l.nvr_graph_launch(g, st))
        nvr.check(l.nvr_stream_synchronize(st))
        for rnd in range(3):
            row = []
            for rn, g in graphs.items():
                l.nvr_event_record(a, st)
                for _ in range(replays):
                    nvr.check(l.nvr_graph_launch(g, st))
                l.nvr_event_record(b, st)
                ms = C.c_float(); nvr.check(l.nvr_event_elapsed_ms(a, b, C.byref(ms)))
                us = ms.value * 1e3 / (replays * L)
                row.append(f"{rn} {us:.2f} us ({rows * K * (1 if rn == 'fp8' else 2) / us / 1e6:.2f} TB/s)")
            print(f"{name} K={K} N={N} T={T} (L={L}, S={S}) round {rnd}: " + ", ".join(row), flush=True)
        for g in graphs.values():
            l.nvr_graph_destroy(g)
    l.nvr_stream_destroy(st)


def head_times(K, N=151936, replays=20):
    st = C.c_void_p(); nvr.check(l.nvr_stream_create(C.byref(st)))
    L = max(4, -(-(768 << 20) // (N * K)))
    x, pv, pi, np_ = nvr.DeviceBuffer(64 * K * 2), nvr.DeviceBuffer(2048 * 64 * 4), nvr.DeviceBuffer(2048 * 64 * 4), C.c_int32(0)
    nvr.check(l.nvr_fill_weight(x.ptr, 64, K, K, K, 0, 0, 3, 1e-5, None))
    W, Wt, Wq, Ws = [], [], [], []
    for i in range(L):
        w, t, q, s = nvr.DeviceBuffer(N * K * 2), nvr.DeviceBuffer(N * K * 2), nvr.DeviceBuffer(N * K), nvr.DeviceBuffer(N * 4)
        nvr.check(l.nvr_fill_weight(w.ptr, N, K, K, K, 0, 0, 5 + i, 1e-6, None))
        nvr.check(l.nvr_retile_weight(w.ptr, t.ptr, N, K, 0, 0, 0, 0, None))
        nvr.check(l.nvr_weight_quantize_fp8(w.ptr, N, K, q.ptr, s.ptr, None, None))
        W.append(w); Wt.append(t); Wq.append(q); Ws.append(s)
    nvr.synchronize()
    a, b = C.c_void_p(), C.c_void_p(); l.nvr_event_create(C.byref(a)); l.nvr_event_create(C.byref(b))
    for T in (1, 32, 64):
        routes = {"fp8": lambda i: l.nvr_lm_head_fp8(x.ptr, K, Wq[i].ptr, Ws[i].ptr, T, K, N, None, pv.ptr, pi.ptr, C.byref(np_), st),
                  "16bit": (lambda i: l.nvr_lm_head_tiled(x.ptr, K, W[i].ptr, Wt[i].ptr, T, K, N, None, pv.ptr, pi.ptr, C.byref(np_), st)) if T <= 32 else
                           (lambda i: l.nvr_lm_head(x.ptr, K, W[i].ptr, T, K, N, None, pv.ptr, pi.ptr, C.byref(np_), st))}
        graphs = {}
        for rn, fn in routes.items():
            nvr.check(fn(0)); nvr.check(l.nvr_stream_synchronize(st))                      # (first call outside the capture: LDS opt-ins)
            nvr.check(l.nvr_graph_capture_begin(st))
            for i in range(L):
                nvr.check(fn(i))
            g = C.c_void_p(); nvr.check(l.nvr_graph_capture_end(st, C.byref(g))); graphs[rn] = g
            for _ in range(2):
                nvr.check(l.nvr_graph_launch(g, st))
        nvr.check(l.nvr_stream_synchronize(st))
        for rnd in range(3):
            row = []
            for rn, g in graphs.items():
                l.nvr_event_record(a, st)
                for _ in range(replays):
                    nvr.check(l.nvr_graph_launch(g, st))
                l.nvr_event_record(b, st)
                ms = C.c_float(); nvr.check(l.nvr_event_elapsed_ms(a, b, C.byref(ms)))
                us = ms.value * 1e3 / (replays * L)
                row.append(f"{rn} {us:.2f} us ({N * K * (1 if rn == 'fp8' else 2) / us / 1e6:.2f} TB/s)")
            print(f"lm_head K={K} N={N} T={T} (L={L}) round {rnd}: " + ", ".join(row), flush=True)
        for g in graphs.values():
            l.nvr_graph_destroy(g)
    l.nvr_stream_destroy(st)


def engine_step_ms(dw, nseq=32, steps=24, preset="qwen3-8b"):
    mc = nvr.ModelConfig(preset)
    eng = nvr.LLMEngine(nvr.Config(max_num_seqs=nseq, max_num_batched_tokens=4096, max_model_len=512, kvcache_block_size=256, num_kvcache_blocks=nseq * 2 + 16,
                                   async_decode=1, decode_weight_dtype=dw), mc)
    for i in range(nseq):
        eng.add_request(nvr.synthetic_tokens(64, 1, i, mc.c.vocab_size).tolist(), nvr.SamplingParams(temperature=0.0, max_tokens=steps + 12, ignore_eos=True))
    while eng.step()["is_prefill"]:
        pass
    for _ in range(4):
        eng.step()
    nvr.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        eng.step()
    nvr.synchronize(); dt = (time.perf_counter() - t0) / steps
    res = (eng.model_runner.decode_weight_dtype(), dt * 1e3)
    del eng
    gc.collect()
    return res


if "kernel" in what:
    for shape in SHAPES:
        kernel_times(*shape)
        gc.collect()
if "engine" in what:
    for rnd in range(2):
        print(f"round {rnd}: " + ", ".join("decode weights %s: %.3f ms per step" % engine_step_ms(dw) for dw in ("auto", "fp8")), flush=True)
if "head" in what:
    for K in (1024, 4096):
        head_times(K)
        gc.collect()
if "head_engine" in what:
    for preset in ("qwen3-0.6b", "qwen3-8b"):
        for nseq in (1, 32):
            for rnd in range(2):
                print(f"{preset} {nseq} sequences round {rnd}: " + ", ".join("decode weights %s: %.3f ms per step" % engine_step_ms(dw, nseq, 24, preset)
                                                                             for dw in ("fp8", "fp8_head")), flush=True)
