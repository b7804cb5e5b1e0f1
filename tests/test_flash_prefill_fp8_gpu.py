"""GPU tests (-m gpu) of the paged MFMA prefill attention over the FP8 (e4m3fn) KV cache (kernels/flash_prefill_fp8.hip), both 16-bit builds:
nvr_attn_prefill_paged_fp8 against oracle.attn_paged on the dequantised caches (table[byte] * scale: exact in f32), and its refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import nvr_import
import oracle
from test_kv_fp8_gpu import E4M3, dev, dtype, e4m3_encode, to16  # noqa: F401  (dtype: the fixture that selects the build)

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _prefill_case(H, KVH, D, bs, cases, scales):
    """byte caches (garbage with NaN codes behind every context), q (values both 16-bit types hold exactly), block tables (a permutation of the pool, -1 past
    each context) and the oracle's result on the dequantised caches: computed once, shared by both builds"""
    rng = np.random.default_rng(29)
    ks, vs = scales
    ctxs, nqs = [c for c, _ in cases], [n for _, n in cases]
    nbs = [(c + bs - 1) // bs for c in ctxs]
    NB, max_blocks = sum(nbs) + 3, max(nbs) + 1
    pool = rng.standard_normal(1 << 16)
    kb = e4m3_encode(pool / ks)[rng.integers(0, pool.size, (NB, bs, KVH, D))]
    vb = e4m3_encode(pool / vs)[rng.integers(0, pool.size, (NB, bs, KVH, D))]
    bt = -np.ones((len(cases), max_blocks), np.int32)
    perm, o = rng.permutation(NB), 0
    for b, c in enumerate(ctxs):
        bt[b, :nbs[b]] = perm[o:o + nbs[b]]; o += nbs[b]
        tail = slice(c % bs, bs) if c % bs else slice(0, 0)
        for cache in (kb, vb):
            g = rng.integers(0, 256, cache[bt[b, nbs[b] - 1], tail].shape).astype(np.uint8)
            g[..., ::3] = 0x7F
            cache[bt[b, nbs[b] - 1], tail] = g
    q = oracle.round_bf16(rng.standard_normal((sum(nqs), H, D)).astype(np.float32))
    q[np.abs(q) < 2.0 ** -10] = 0                                # (smaller bf16 values are not fp16 values)
    cu = np.concatenate([[0], np.cumsum(nqs)]).astype(np.int32)
    ctx = np.asarray(ctxs, np.int32)
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    ref = oracle.attn_paged(q, cu, np.nan_to_num(E4M3[kb] * np.float32(ks)), np.nan_to_num(E4M3[vb] * np.float32(vs)), bt, ctx, scale)
    return kb, vb, bt, max_blocks, q, cu, ctx, scale, ref


@pytest.mark.parametrize("H,KVH,D,bs,cases,scales", [
    (4, 2, 64, 64, ((150, 22), (150, 150), (200, 60), (64, 1)), (1.0, 1.0)),   # D=64, G=2, block = key step; prefix + new, all new, a query at a block edge
    (16, 8, 128, 128, ((700, 130), (129, 129)), (1.0, 1.0)),                    # D=128, more than one query tile per sequence
    (16, 8, 128, 128, ((700, 130), (129, 129)), (0.25, 4.0)),                   # ... with scales
    (8, 2, 128, 256, ((300, 44),), (1.0, 1.0)),                                 # G=4, the engine's block size
    (4, 4, 128, 64, ((65, 65), (191, 1)), (1.0, 1.0)),                          # G=1, one key past a step, a decode-like row
    (4, 1, 64, 64, ((100, 37),), (1.0, 1.0)),                                   # D=64, G=4
    (4, 2, 64, 64, ((4200, 5),), (1.0, 1.0)),                                   # more than 64 block-table entries: a second register copy of the table
])
def test_fp8_paged_prefill_attention(dtype, H, KVH, D, bs, cases, scales):
    kb, vb, bt, max_blocks, q, cu, ctx, scale, ref = _prefill_case(H, KVH, D, bs, cases, scales)
    T, B = int(cu[-1]), len(cases)
    meta = nvr.AttnMetaC()
    d_cu, d_ctx, d_bt = dev(cu), dev(ctx), dev(bt)
    meta.is_prefill, meta.cu_seqlens_q, meta.context_lens, meta.block_tables = 1, d_cu.ptr, d_ctx.ptr, d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = max_blocks, B, int(ctx.max())
    d_out = dev(np.zeros((T, H, D), np.uint16))
    nvr.check(nvr.lib().nvr_attn_prefill_paged_fp8(dev(to16(q, dtype)[1]).ptr, H * D, dev(kb).ptr, dev(vb).ptr, C.byref(meta), T, H, KVH, D, bs,
                                                   scale, scales[0], scales[1], d_out.ptr, None))
    u, want = d_out.to_numpy((T, H, D), np.uint16), to16(ref, dtype)[0]
    got = (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)
    # exact inputs, the 16-bit flash kernel's rounding points (P to 16 bits in front of the second MFMA), so its bounds: 2 ulp + 2e-3 (fp16,
    # test_attn_prefill_paged_prefix) / 2 ulp + 1.6e-2 (bf16, test_attn_prefill_varlen of test_kernels_bf16_gpu.py)
    err = np.abs(got - want)
    print(f"max |err| {err.max():.3e}")
    tol = (1.6e-2 + 2 * np.abs(want) * 2.0 ** -7) if dtype == "bfloat16" else (2e-3 + 2 * np.abs(want) * 2.0 ** -10)
    assert np.isfinite(got).all(), "a NaN byte behind a context reached the output"                  # (NaN > tol is False: its own assertion)
    assert not (err > tol).any(), f"{(err > tol).sum()} / {err.size} elements off, max err {err.max()}"


@pytest.mark.parametrize("dtype,H,KVH,D,bs", [("float16", 4, 2, 64, 16), ("float16", 4, 2, 64, 48), ("float16", 4, 2, 96, 64), ("bfloat16", 16, 2, 128, 64),
                                              ("float32", 8, 8, 128, 64)], indirect=["dtype"])
def test_fp8_paged_prefill_unsupported_requests(dtype, H, KVH, D, bs):
    """block sizes 16 and 48, D=96, G=8 and the float32 ops all answer NVR_ERR_UNSUPPORTED before anything is launched"""
    buf = dev(np.zeros(64 * 1024, np.uint8))
    meta = nvr.AttnMetaC()
    meta.is_prefill, meta.cu_seqlens_q, meta.context_lens, meta.block_tables = 1, buf.ptr, buf.ptr, buf.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = 2, 1, 16
    assert nvr.lib().nvr_attn_prefill_paged_fp8(buf.ptr, H * D, buf.ptr, buf.ptr, C.byref(meta), 0, H, KVH, D, bs, 0.1, 1.0, 1.0, buf.ptr, None) == -10
