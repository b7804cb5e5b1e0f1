"""GPU tests (-m gpu) of the work-balanced decode attention over the FP8 KV cache (attn_share_fp8_kernel, kernels/attention_fp8.hip), both 16-bit builds:
nvr_paged_attn_decode_fp8 with tickets, at pair counts the launch rule selects on 256 CUs (264 and 280 pairs), against oracle.attn_decode on the dequantised caches."""
import ctypes as C

import numpy as np
import pytest

import nvr_import
from test_kv_fp8_gpu import _decode_case, dev, dtype, to16  # noqa: F401  (dtype: the fixture)

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,KVH,D,bs,ctxs,scales", [
    (33, 16, 8, 128, 256, tuple(1 + (389 * i) % 2000 for i in range(33)), (1.0, 1.0)),   # G=2: one-key contexts, pairs cut by several share boundaries
    (33, 16, 8, 128, 256, tuple(1 + (389 * i) % 2000 for i in range(33)), (0.25, 4.0)),  # ... with scales
    (33, 8, 8, 128, 16, tuple(1 + (389 * i) % 2000 for i in range(33)), (1.0, 1.0)),     # G=1, the smallest block at D=128, > 64 block-table entries
    (70, 16, 4, 64, 64, tuple(1 + (613 * i) % 4300 for i in range(70)), (1.0, 1.0)),     # G=4, D=64, > 64 block-table entries
])
def test_fp8_work_balanced_attn_decode(dtype, B, H, KVH, D, bs, ctxs, scales):
    """measured max |err| over the cases (MI355X): 2.4e-4 in the fp16 build, 9.8e-4 in the bf16 build"""
    kb, vb, bt, max_blocks, q, ctx, scale, ref = _decode_case(B, H, KVH, D, bs, ctxs, scales)
    meta = nvr.AttnMetaC()
    d_ctx, d_bt = dev(ctx), dev(bt)
    meta.is_prefill, meta.context_lens, meta.block_tables = 0, d_ctx.ptr, d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = max_blocks, B, int(max(ctxs))
    ws = nvr.DeviceBuffer(nvr.lib().nvr_paged_attn_workspace_bytes(B, H, D, int(max(ctxs))))
    tickets = dev(np.zeros(B * KVH, np.uint32))
    d_q, d_k, d_v = dev(to16(q, dtype)[1]), dev(kb), dev(vb)

    def launch():
        d_out = dev(np.full((B, H, D), 0x7E7E, np.uint16))
        nvr.check(nvr.lib().nvr_paged_attn_decode_fp8(d_q.ptr, H * D, d_k.ptr, d_v.ptr, C.byref(meta), H, KVH, D, bs, scale, scales[0], scales[1], d_out.ptr,
                                                      ws.ptr, tickets.ptr, None))
        return d_out.to_numpy((B, H, D), np.uint16)
    want = to16(ref, dtype)[0]
    tol = 1e-3 + 2 * np.abs(want) * 2.0 ** (-7 if dtype == "bfloat16" else -10)           # the fp8 decode tests' bound

    def check(u, rows):
        got = (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)
        err = np.abs(got - want)[rows]
        print(f"max |err| {np.nanmax(err):.3e}")
        bad = ~(err <= tol[rows])                                                          # (a NaN — the fill of a row nobody wrote, in fp16 — is off too)
        assert not bad.any(), f"{bad.sum()} / {err.size} elements off, max err {np.nanmax(err)}"
    u = launch()
    check(u, np.arange(B))
    assert np.array_equal(launch(), u), "a second launch on the same tickets differs in bits (re-arm / merge order)"
    if scales == (1.0, 1.0) and bs == 256:                                                 # a query without keys owns no unit and still gets a zero row
        ctx0 = ctx.copy(); ctx0[5] = 0
        d_ctx0 = dev(ctx0); meta.context_lens = d_ctx0.ptr
        z = launch()
        assert not z[5].any(), "the row of the query without keys is not zero"
        check(z, np.arange(B) != 5)
