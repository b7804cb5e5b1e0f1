"""GPU tests (-m gpu) of the FP8 (e4m3fn) KV cache kernels (kernels/attention_fp8.hip), both 16-bit builds: nvr_kv_store_fp8 against a numpy encoder
(bytes exact), nvr_paged_attn_decode_fp8 against oracle.attn_decode on the dequantised caches (table[byte] * scale: exact in f32)."""
import ctypes as C
import functools

import numpy as np
import pytest

import nvr_import
import oracle

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu
_KEEP = []
_b = np.arange(256)                                 # value of every e4m3fn byte from its bit fields (bias 7, subnormals at exponent 0; 0x7F / 0xFF: NaN)
E4M3 = (np.where(_b & 0x78, (1 + (_b & 7) / 8.0) * 2.0 ** (((_b >> 3) & 15) - 7.0), (_b & 7) / 8.0 * 2.0 ** -6) * np.where(_b & 0x80, -1.0, 1.0)).astype(np.float32)
E4M3[[0x7F, 0xFF]] = np.nan
_POS = E4M3[:0x7F].astype(np.float64)               # the finite non-negative codes 0 .. 0x7E, ascending


def e4m3_encode(x):
    """round to nearest, ties to the even mantissa, clamped to +-448"""
    x = np.asarray(x, np.float64); a = np.minimum(np.abs(x), 448.0)
    hi = np.clip(np.searchsorted(_POS, a, side="left"), 1, 0x7E); lo = hi - 1
    dl, dh = a - _POS[lo], _POS[hi] - a
    code = np.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


@pytest.fixture(params=["float16", "bfloat16"])
def dtype(request):
    nvr.check(nvr.lib().nvr_device_set(0))
    nvr.check(nvr.lib().nvr_ops_set_dtype(request.param.encode()))
    yield request.param
    nvr.synchronize()
    _KEEP.clear()
    nvr.check(nvr.lib().nvr_ops_set_dtype(b"float16"))


def dev(a):
    b = nvr.DeviceBuffer.from_numpy(np.ascontiguousarray(a))
    _KEEP.append(b)
    return b


def to16(a, dtype):
    """values rounded to the 16-bit type (as f32) and their bit patterns"""
    f = oracle.round_bf16(np.asarray(a, np.float32)) if dtype == "bfloat16" else np.asarray(a, np.float32).astype(np.float16)
    return (f, oracle.to_bf16_bits(f)) if dtype == "bfloat16" else (f.astype(np.float32), f.view(np.uint16))


@pytest.mark.parametrize("ks,vs", [(1.0, 1.0), (0.5, 2.0)])
@pytest.mark.parametrize("D,KVH,T", [(64, 2, 5), (128, 8, 33)])
def test_fp8_store_bytes_exact(dtype, D, KVH, T, ks, vs):
    rng = np.random.default_rng(11)
    H, bs, NB = 2 * KVH, 16, 4
    x = rng.standard_normal((T, (H + 2 * KVH) * D)) * 3
    ties = [(_POS[k] + _POS[k + 1]) / 2 for k in (0, 1, 2, 8, 9, 0x40, 0x41, 0x7D)]
    for col0, sc in ((H * D, ks), ((H + KVH) * D, vs)):         # planted in the K and in the V columns of rows 0 and 1
        plant = np.asarray([448 * sc, -448 * sc, 1000, -1000, 2.0 ** -9 * sc, -2.0 ** -9 * sc] + [t * sc for t in ties] + [-t * sc for t in ties])
        x[0, col0:col0 + plant.size] = plant
        x[1, col0 + 3:col0 + 3 + plant.size] = plant
    xf, xb = to16(x, dtype)
    slots = rng.permutation(NB * bs)[:T].astype(np.int32)
    slots[2] = -1
    d_k, d_v = dev(np.zeros((NB * bs, KVH * D), np.uint8)), dev(np.zeros((NB * bs, KVH * D), np.uint8))
    nvr.check(nvr.lib().nvr_kv_store_fp8(dev(xb).ptr, dev(slots).ptr, T, H, KVH, D, ks, vs, d_k.ptr, d_v.ptr, None))
    for buf, col0, sc, what in ((d_k, H * D, ks, "K"), (d_v, (H + KVH) * D, vs, "V")):
        want = np.zeros((NB * bs, KVH * D), np.uint8)            # rows no slot addresses stay 0
        want[slots[slots >= 0]] = e4m3_encode(xf[slots >= 0, col0:col0 + KVH * D].astype(np.float64) / sc)
        got = buf.to_numpy((NB * bs, KVH * D), np.uint8)
        assert np.array_equal(got, want), f"{what} cache: {(got != want).sum()} bytes differ from the reference encoder"


@functools.lru_cache(maxsize=None)
def _decode_case(B, H, KVH, D, bs, ctxs, scales):
    """byte caches, q (values both 16-bit types hold exactly) and the oracle's result on the dequantised caches: computed once, shared by both builds"""
    rng = np.random.default_rng(6)
    ks, vs = scales
    nbs = [(c + bs - 1) // bs for c in ctxs]
    NB, max_blocks = sum(nbs) + 3, max(nbs) + 1
    pool = rng.standard_normal(1 << 16)                          # (a pool: encoding every cache element would take seconds at the largest case)
    kb = e4m3_encode(pool / ks)[rng.integers(0, pool.size, (NB, bs, KVH, D))]
    vb = e4m3_encode(pool / vs)[rng.integers(0, pool.size, (NB, bs, KVH, D))]
    bt = -np.ones((B, max_blocks), np.int32)
    perm, o = rng.permutation(NB), 0
    for b, c in enumerate(ctxs):
        bt[b, :nbs[b]] = perm[o:o + nbs[b]]; o += nbs[b]
        tail = slice(c % bs, bs) if c % bs else slice(0, 0)   # behind the context inside the last block: garbage, NaN bytes included
        for cache in (kb, vb):
            g = rng.integers(0, 256, cache[bt[b, nbs[b] - 1], tail].shape).astype(np.uint8)
            g[..., ::3] = 0x7F
            cache[bt[b, nbs[b] - 1], tail] = g
    q = oracle.round_bf16(rng.standard_normal((B, H, D)).astype(np.float32))
    q[np.abs(q) < 2.0 ** -10] = 0                                # (smaller bf16 values are not fp16 values)
    ctx = np.asarray(ctxs, np.int32)
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    ref = oracle.attn_decode(q, np.nan_to_num(E4M3[kb] * np.float32(ks)), np.nan_to_num(E4M3[vb] * np.float32(vs)), bt, ctx, scale)
    return kb, vb, bt, max_blocks, q, ctx, scale, ref


@pytest.mark.parametrize("B,H,KVH,D,bs,ctxs,scales", [
    (3, 4, 2, 64, 16, (1, 17, 40), (1.0, 1.0)),                  # D=64, partial row groups, a one-key context
    (4, 16, 8, 128, 256, (1, 255, 256, 700), (1.0, 1.0)),        # the Qwen3-0.6B heads, block edges
    (4, 16, 8, 128, 256, (1, 255, 256, 700), (0.25, 4.0)),       # ... with scales
    (2, 32, 8, 128, 256, (513, 1024), (1.0, 1.0)),               # G=4
    (5, 8, 8, 128, 16, (5, 16, 31, 32, 33), (1.0, 1.0)),         # G=1, blocks of one chunk
    (1, 16, 8, 128, 256, (3000,), (1.0, 1.0)),                   # many partitions and the merge
    (3, 4, 2, 128, 16, (2500, 1030, 7), (1.0, 1.0)),             # more than 64 block-table entries
    (300, 16, 8, 128, 64, tuple(1 + (41 * i) % 250 for i in range(300)), (1.0, 1.0)),   # the many-pairs launch shape
])
def test_fp8_paged_attn_decode(dtype, B, H, KVH, D, bs, ctxs, scales):
    kb, vb, bt, max_blocks, q, ctx, scale, ref = _decode_case(B, H, KVH, D, bs, ctxs, scales)
    meta = nvr.AttnMetaC()
    d_ctx, d_bt = dev(ctx), dev(bt)
    meta.is_prefill, meta.context_lens, meta.block_tables = 0, d_ctx.ptr, d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = max_blocks, B, int(max(ctxs))
    ws = nvr.DeviceBuffer(nvr.lib().nvr_paged_attn_workspace_bytes(B, H, D, int(max(ctxs))))
    d_out = nvr.DeviceBuffer(B * H * D * 2)
    nvr.check(nvr.lib().nvr_paged_attn_decode_fp8(dev(to16(q, dtype)[1]).ptr, H * D, dev(kb).ptr, dev(vb).ptr, C.byref(meta), H, KVH, D, bs,
                                                  scale, scales[0], scales[1], d_out.ptr, ws.ptr, None, None))
    u, want = d_out.to_numpy((B, H, D), np.uint16), to16(ref, dtype)[0]
    got = (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)
    # the 16-bit decode tests' bound: 2 ulp of the 16-bit type + 1e-3 (f32 online softmax vs two-pass softmax on exact inputs)
    err = np.abs(got - want)
    print(f"max |err| {err.max():.3e}")
    tol = 1e-3 + 2 * np.abs(want) * 2.0 ** (-7 if dtype == "bfloat16" else -10)
    assert not (err > tol).any(), f"{(err > tol).sum()} / {err.size} elements off, max err {err.max()}"


@pytest.mark.parametrize("dtype,H,KVH,D", [("float16", 4, 2, 96), ("bfloat16", 16, 2, 128), ("float32", 8, 8, 128)], indirect=["dtype"])
def test_fp8_unsupported_requests(dtype, H, KVH, D):
    """D=96, G=8 and the float32 ops (a supported head shape) all answer NVR_ERR_UNSUPPORTED before anything is launched"""
    buf = dev(np.zeros(64 * 1024, np.uint8))
    meta = nvr.AttnMetaC()
    meta.context_lens, meta.block_tables, meta.max_blocks, meta.batch, meta.max_context_len = buf.ptr, buf.ptr, 2, 1, 16
    assert nvr.lib().nvr_paged_attn_decode_fp8(buf.ptr, H * D, buf.ptr, buf.ptr, C.byref(meta), H, KVH, D, 16, 0.1, 1.0, 1.0, buf.ptr, None, None, None) == -10
    if dtype == "float32":
        assert nvr.lib().nvr_kv_store_fp8(buf.ptr, buf.ptr, 1, H, KVH, D, 1.0, 1.0, buf.ptr, buf.ptr, None) == -10
