"""flash prefill alone: B sequences x L tokens of Qwen3-0.6B geometry (H 16, KVH 8, D 128), HIP-event timing (median) — for A/B of
library builds (NVR_LIBNVR=...) and counter passes.  python tools/flash_bench.py [L] [H] [KVH] [reps] [--paged fp16|fp8|both]
--paged: the same queries through block tables of size 256 over 16-bit caches (nvr_attn_prefill_paged), e4m3 byte caches
(nvr_attn_prefill_paged_fp8) or both in alternation; every launch of a kind reads its own cache set (8 sets, 134 / 67 MB each: nothing is
re-read from the infinity cache).  The entry points build their tile list per call (allocation, copy, synchronise), so the event times of the
paged forms contain that host work: take kernel times from a rocprofv3 --kernel-trace --stats run of this script."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, nvr_import
nvr = nvr_import.load(); l = nvr.lib(); nvr.check(l.nvr_device_set(0))
args = list(sys.argv[1:])
paged = args.pop(args.index("--paged") + 1) if "--paged" in args else None
if paged: args.remove("--paged")
L = int(args[0]) if len(args) > 0 else 1024
H = int(args[1]) if len(args) > 1 else 16
KVH = int(args[2]) if len(args) > 2 else 8
reps = int(args[3]) if len(args) > 3 else 12
D, T = 128, 32768
B = T // L
st = C.c_void_p(); l.nvr_stream_create(C.byref(st))
QKV = (H + 2 * KVH) * D
y = nvr.DeviceBuffer(T * QKV * 2); nvr.check(l.nvr_fill_weight(y.ptr, 1, T * QKV, T * QKV, T * QKV, 0, 0, 7, 0.02, None))
cu = nvr.DeviceBuffer.from_numpy((np.arange(B + 1) * L).astype(np.int32))
meta = nvr.AttnMetaC(); meta.is_prefill = 1; meta.cu_seqlens_q = cu.ptr; meta.cu_seqlens_k = cu.ptr; meta.max_seqlen_q = L; meta.max_seqlen_k = L; meta.batch = B
out = nvr.DeviceBuffer(T * H * D * 2)
qp = y.ptr; kp = y.ptr + H * D * 2; vp = y.ptr + (H + KVH) * D * 2
scale = float(1 / np.sqrt(D))
fl = 4 * H * D * B * (L * (L + 1) // 2)


def timed(what, launch):
    evs = []
    for rep in range(reps):
        a, b = C.c_void_p(), C.c_void_p(); l.nvr_event_create(C.byref(a)); l.nvr_event_create(C.byref(b))
        l.nvr_event_record(a, st)
        nvr.check(launch(rep))
        l.nvr_event_record(b, st); evs.append((a, b))
    nvr.check(l.nvr_stream_synchronize(st)); ts = []
    for a, b in evs:
        ms = C.c_float(); nvr.check(l.nvr_event_elapsed_ms(a, b, C.byref(ms))); ts.append(ms.value * 1e3)
    ts = sorted(ts[2:]); us = ts[len(ts) // 2]
    print(f"flash {what} {B} x {L} H={H} KVH={KVH}: {us:8.1f} us (min {ts[0]:.1f})  {fl/us/1e6:7.1f} TF/s causal  lib={os.environ.get('NVR_LIBNVR','default')}")


if not paged:
    timed("varlen", lambda rep: l.nvr_attn_prefill_varlen(qp, kp, vp, QKV, C.byref(meta), T, H, KVH, D, scale, out.ptr, st))
else:
    BS, SETS = 256, 8
    nb = (L + BS - 1) // BS                                          # blocks per sequence; the pool is exactly B * nb blocks, handed out in a shuffled order
    rng = np.random.default_rng(3)
    bt = nvr.DeviceBuffer.from_numpy(rng.permutation(B * nb).astype(np.int32).reshape(B, nb))
    ctx = nvr.DeviceBuffer.from_numpy(np.full(B, L, np.int32))
    meta.context_lens, meta.block_tables, meta.max_blocks, meta.max_context_len = ctx.ptr, bt.ptr, nb, L
    n = B * nb * BS * KVH * D                                        # elements of one cache
    kinds = ["fp16", "fp8"] if paged == "both" else [paged]
    sets = {}
    for kind in kinds:
        sets[kind] = []
        for s in range(SETS):
            if kind == "fp16":
                kc, vc = nvr.DeviceBuffer(n * 2), nvr.DeviceBuffer(n * 2)
                nvr.check(l.nvr_fill_weight(kc.ptr, 1, n, n, n, 0, 0, 11 + 2 * s, 0.02, None)); nvr.check(l.nvr_fill_weight(vc.ptr, 1, n, n, n, 0, 0, 12 + 2 * s, 0.02, None))
            else:                                                    # random finite e4m3 codes of |value| < 2 (exponent field <= 7)
                kc, vc = (nvr.DeviceBuffer.from_numpy(rng.integers(0, 256, n, dtype=np.uint8) & 0xBF) for _ in range(2))
            sets[kind].append((kc, vc))
    nvr.synchronize()
    for round_ in range(2 if paged == "both" else 1):                # alternating rounds
        for kind in kinds:
            if kind == "fp16":
                timed("paged fp16", lambda rep: l.nvr_attn_prefill_paged(qp, QKV, sets["fp16"][rep % SETS][0].ptr, sets["fp16"][rep % SETS][1].ptr, C.byref(meta), T, H, KVH, D, BS,
                                                                         scale, out.ptr, st))
            else:
                timed("paged fp8 ", lambda rep: l.nvr_attn_prefill_paged_fp8(qp, QKV, sets["fp8"][rep % SETS][0].ptr, sets["fp8"][rep % SETS][1].ptr, C.byref(meta), T, H, KVH, D, BS,
                                                                             scale, 1.0, 1.0, out.ptr, st))
