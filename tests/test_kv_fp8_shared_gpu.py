"""GPU tests (-m gpu) of the shared-prefix decode attention over the FP8 (e4m3fn) KV cache (nvr_paged_attn_decode_shared_fp8), both 16-bit builds,
against oracle.attn_decode on the dequantised caches."""
import ctypes as C
import functools

import numpy as np
import pytest

import nvr_import
import oracle
from test_kv_fp8_gpu import E4M3, dev, dtype, e4m3_encode, to16  # noqa: F401  (dtype: the fixture)

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(B, H, KVH, D, bs, P, ctxs, members, scales):
    """byte caches whose first P blocks are the same for every member, garbage (NaN bytes included) behind each context, q, and the oracle's result"""
    rng = np.random.default_rng(8)
    ks, vs = scales
    nbs = [(c + bs - 1) // bs for c in ctxs]
    NB, max_blocks = P + sum(nbs) + 3, max(nbs) + 1
    pool = rng.standard_normal(1 << 16)
    kb = e4m3_encode(pool / ks)[rng.integers(0, pool.size, (NB, bs, KVH, D))]
    vb = e4m3_encode(pool / vs)[rng.integers(0, pool.size, (NB, bs, KVH, D))]
    bt = -np.ones((B, max_blocks), np.int32)
    perm = rng.permutation(NB)
    shared, o = perm[:P], P
    for b, c in enumerate(ctxs):
        own = nbs[b] - (P if b in members else 0)
        bt[b, :nbs[b]] = np.concatenate([shared if b in members else perm[:0], perm[o:o + own]]); o += own
        if c % bs:                                               # behind the context inside its last block (never a shared block: those are full)
            for cache in (kb, vb):
                g = rng.integers(0, 256, cache[bt[b, nbs[b] - 1], c % bs:].shape).astype(np.uint8)
                g[..., ::3] = 0x7F
                cache[bt[b, nbs[b] - 1], c % bs:] = g
    q = oracle.round_bf16(rng.standard_normal((B, H, D)).astype(np.float32))
    q[np.abs(q) < 2.0 ** -10] = 0                                # (smaller bf16 values are not fp16 values)
    ctx = np.asarray(ctxs, np.int32)
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    ref = oracle.attn_decode(q, np.nan_to_num(E4M3[kb] * np.float32(ks)), np.nan_to_num(E4M3[vb] * np.float32(vs)), bt, ctx, scale)
    return kb, vb, bt, max_blocks, q, ctx, scale, ref


def _all(B, H, KVH, D, bs, P, own, scales):
    return B, H, KVH, D, bs, P, tuple(P * bs + int(x) for x in own), tuple(range(B)), scales


CASES = [
    _all(5, 4, 2, 64, 64, 1, [0, 1, 63, 64, 130], (1.0, 1.0)),                              # D = 64, G = 2, members with no own keys, partial blocks
    _all(2, 16, 8, 128, 256, 1, [0, 0], (1.0, 1.0)),                                        # only the shared partition exists
    _all(70, 16, 8, 128, 256, 2, np.random.default_rng(1).integers(0, 300, 70), (0.25, 4.0)),   # configs[4] heads, several shared partitions, scales
    _all(130, 8, 8, 128, 64, 3, [(7 * i) % 200 for i in range(130)], (1.0, 1.0)),           # G = 1: a full 128-row tile and a ragged last tile
    _all(33, 8, 2, 128, 128, 1, [5 + i for i in range(33)], (1.0, 1.0)),                    # G = 4
    _all(4, 4, 2, 64, 64, 65, [3, 0, 64, 17], (1.0, 1.0)),                                  # a shared prefix of more than 64 block-table entries
    # a group of 6 scattered through a batch of 9; the others (contexts 1, P*bs - 5, P*bs + 70) sit on blocks of their own
    (9, 4, 2, 128, 64, 2, (1, 128 + 9, 128, 128 - 5, 128 + 64, 128 + 131, 128 + 70, 128 + 1, 128 + 40), (1, 2, 4, 5, 7, 8), (0.5, 2.0)),
]


def _call(dtype, case, shared_len=None, bs=None, rows="auto", kv0="auto"):
    B, H, KVH, D, bs0, P, ctxs, members, scales = case
    kb, vb, bt, max_blocks, q, ctx, scale, ref = _case(*case)
    meta = nvr.AttnMetaC()
    d_ctx, d_bt = dev(ctx), dev(bt)
    meta.is_prefill, meta.context_lens, meta.block_tables = 0, d_ctx.ptr, d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = max_blocks, B, int(max(ctxs))
    ws = nvr.DeviceBuffer(nvr.lib().nvr_paged_attn_workspace_bytes(B, H, D, int(max(ctxs)) + P * bs0 + bs0))
    d_out = nvr.DeviceBuffer(B * H * D * 2)
    grp = len(members) < B
    d_rows = dev(np.asarray(list(members) + [members[0]] * (B - len(members)), np.int32)).ptr if (grp if rows == "auto" else rows) else None
    d_kv0 = dev(np.asarray([P * bs0 if b in members else 0 for b in range(B)], np.int32)).ptr if (grp if kv0 == "auto" else kv0) else None
    d_cnt = dev(np.asarray([len(members)], np.int32)).ptr if grp else None
    rc = nvr.lib().nvr_paged_attn_decode_shared_fp8(dev(to16(q, dtype)[1]).ptr, H * D, dev(kb).ptr, dev(vb).ptr, C.byref(meta), H, KVH, D, bs or bs0, scale,
                                                    scales[0], scales[1], P * bs0 if shared_len is None else shared_len, d_rows, d_kv0, d_cnt, d_out.ptr, ws.ptr, None)
    return rc, d_out, ref


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-H{c[1]}-KVH{c[2]}-D{c[3]}-bs{c[4]}-P{c[5]}" for c in CASES])
def test_fp8_paged_attn_decode_shared_prefix(dtype, case):
    """measured max |err| (MI355X): fp16 4.9e-4, bf16 2.0e-3 over all cases"""
    B, H, D = case[0], case[1], case[3]
    rc, d_out, ref = _call(dtype, case)
    nvr.check(rc)
    u, want = d_out.to_numpy((B, H, D), np.uint16), to16(ref, dtype)[0]
    got = (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)
    # the bound of test_fp8_paged_prefill_attention (the shared partitions have that kernel's rounding points; the own ones are the decode kernel's)
    err = np.abs(got - want)
    print(f"max |err| {err.max():.3e}")
    tol = (1.6e-2 + 2 * np.abs(want) * 2.0 ** -7) if dtype == "bfloat16" else (2e-3 + 2 * np.abs(want) * 2.0 ** -10)
    assert np.isfinite(got).all(), "a NaN byte behind a context reached the output"
    assert not (err > tol).any(), f"{(err > tol).sum()} / {err.size} elements off, max err {err.max()}"


@pytest.mark.parametrize("dtype", ["float16", "float32"], indirect=True)
def test_fp8_shared_prefix_refusals(dtype):
    """all answered before anything is launched"""
    if dtype == "float32":
        assert _call("float16", CASES[0])[0] == -10
        return
    assert _call(dtype, CASES[0], shared_len=64 + 8)[0] == -7       # not whole blocks
    assert _call(dtype, CASES[0], bs=16)[0] == -10                  # block size below the 64-key step
    assert _call(dtype, CASES[0], rows=True)[0] == -7               # rows without kv0 / count
