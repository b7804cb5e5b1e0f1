"""GPU tests (-m gpu) of the work-balanced MFMA decode attention over the FP8 KV cache at 8 query heads per kv head (attn_share_fp8_mfma_kernel,
kernels/attention_fp8_mfma.hip), both 16-bit builds: nvr_paged_attn_decode_fp8 WITH tickets, at pair counts the pair-count rule selects on 256 CUs (264 and
280 pairs), against oracle.attn_decode on the dequantised caches."""
import ctypes as C

import numpy as np
import pytest

import nvr_import
from test_kv_fp8_gpu import _decode_case, dev, dtype, to16  # noqa: F401  (dtype: the fixture of both builds)

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,KVH,D,bs,ctxs,scales", [
    (132, 16, 2, 128, 64, tuple(1 + (389 * i) % 2000 for i in range(132)), (1.0, 1.0)),   # one-key contexts, pairs cut by several workers and pairs inside one, block edges
    (132, 16, 2, 128, 64, tuple(1 + (389 * i) % 2000 for i in range(132)), (0.25, 4.0)),  # ... both scales, in direct rows and in merged partials
    (70, 32, 4, 64, 64, tuple(1 + (613 * i) % 4300 for i in range(70)), (1.0, 1.0)),      # D = 64, > 64 block-table entries: the register copy reloaded mid-segment
    (132, 16, 2, 128, 256, tuple(0 if i in (3, 64, 131) else 300 if i == 77 else 1 for i in range(132)), (1.0, 1.0)),   # units far below the workers: the clamp, idle workers, zero rows
])
def test_fp8_mfma_work_balanced_attn_decode_gqa8(dtype, B, H, KVH, D, bs, ctxs, scales):
    kb, vb, bt, max_blocks, q, ctx, scale, ref = _decode_case(B, H, KVH, D, bs, ctxs, scales)
    meta = nvr.AttnMetaC()
    d_ctx, d_bt = dev(ctx), dev(bt)
    meta.is_prefill, meta.context_lens, meta.block_tables = 0, d_ctx.ptr, d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = max_blocks, B, int(max(ctxs))
    ws = nvr.DeviceBuffer(nvr.lib().nvr_paged_attn_workspace_bytes(B, H, D, int(max(ctxs))))
    tickets = dev(np.zeros(B * KVH, np.uint32))
    d_q, d_k, d_v = dev(to16(q, dtype)[1]), dev(kb), dev(vb)

    def launch():
        d_out = dev(np.full((B, H, D), 0x7E7E, np.uint16))                                 # (an unwritten row is seen: NaN in fp16, 5e37 in bf16)
        nvr.check(nvr.lib().nvr_paged_attn_decode_fp8(d_q.ptr, H * D, d_k.ptr, d_v.ptr, C.byref(meta), H, KVH, D, bs, scale, scales[0], scales[1], d_out.ptr,
                                                      ws.ptr, tickets.ptr, None))
        return d_out.to_numpy((B, H, D), np.uint16)
    u, want, rows = launch(), to16(ref, dtype)[0], ctx > 0
    got = (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)
    # the MFMA attention bound of test_fp8_mfma_paged_attn_decode_gqa8: 2 ulp of the 16-bit type + 2e-3 (fp16) / 1.6e-2 (bf16), on every element
    err = np.abs(got - want)[rows]
    tol = ((1.6e-2 if dtype == "bfloat16" else 2e-3) + 2 * np.abs(want) * 2.0 ** (-7 if dtype == "bfloat16" else -10))[rows]
    print(f"max |err| {np.nanmax(err):.3e}")
    bad = ~(err <= tol)                                                                     # (a NaN is off too)
    assert not bad.any(), f"{bad.sum()} / {err.size} elements off, max err {np.nanmax(err)}"
    assert not u[~rows].any(), "the row of a query without keys is not zero"
    assert np.array_equal(launch(), u), "a second launch on the same tickets differs in bits (re-arm / merge order)"
