"""GPU tests (-m gpu) of paged decode attention over the FP8 KV cache at 8 query heads per kv head (kernels/attention_fp8_mfma.hip), both 16-bit builds:
nvr_paged_attn_decode_fp8 against oracle.attn_decode on the dequantised caches, NaN bytes planted behind every context (test_kv_fp8_gpu._decode_case)."""
import ctypes as C

import numpy as np
import pytest

import nvr_import
from test_kv_fp8_gpu import _decode_case, dev, dtype, to16  # noqa: F401  (dtype: the fixture of both builds)

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,KVH,D,bs,ctxs,scales", [
    (5, 16, 2, 128, 64, (1, 63, 64, 65, 130), (1.0, 1.0)),       # step and block edges, one key, waves without a step
    (3, 8, 1, 64, 64, (7, 200, 321), (0.25, 4.0)),               # the D = 64 instance, scales
    (1, 16, 2, 128, 256, (3000,), (1.0, 1.0)),                   # split partitions and the merge, a ragged last partition
    (2, 8, 1, 128, 64, (4200, 70), (1.0, 1.0)),                  # more than 64 block-table entries
    (300, 16, 2, 128, 64, tuple(1 + (41 * i) % 250 for i in range(300)), (1.0, 1.0)),   # more workgroups than one round of CUs
])
def test_fp8_mfma_paged_attn_decode_gqa8(dtype, B, H, KVH, D, bs, ctxs, scales):
    kb, vb, bt, max_blocks, q, ctx, scale, ref = _decode_case(B, H, KVH, D, bs, ctxs, scales)
    meta = nvr.AttnMetaC()
    d_bt, d_q, d_k, d_v = dev(bt), dev(to16(q, dtype)[1]), dev(kb), dev(vb)
    meta.is_prefill, meta.block_tables = 0, d_bt.ptr
    meta.max_blocks, meta.batch, meta.max_context_len = max_blocks, B, int(max(ctxs))
    ws = nvr.DeviceBuffer(nvr.lib().nvr_paged_attn_workspace_bytes(B, H, D, int(max(ctxs))))

    def run(ctx_lens):
        d_ctx, d_out = dev(ctx_lens), nvr.DeviceBuffer(B * H * D * 2)
        meta.context_lens = d_ctx.ptr
        nvr.check(nvr.lib().nvr_paged_attn_decode_fp8(d_q.ptr, H * D, d_k.ptr, d_v.ptr, C.byref(meta), H, KVH, D, bs, scale, scales[0], scales[1], d_out.ptr,
                                                      ws.ptr, None, None))
        return d_out.to_numpy((B, H, D), np.uint16)

    u, want = run(ctx), to16(ref, dtype)[0]
    assert np.array_equal(u, run(ctx)), "two launches on the same inputs differ in bits"
    got = (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)
    # the MFMA attention bound (P is rounded to 16 bits in front of P.V): 2 ulp of the 16-bit type + 2e-3 (fp16) / 1.6e-2 (bf16), on every element
    err = np.abs(got - want)
    print(f"max |err| {err.max():.3e}")
    tol = (1.6e-2 if dtype == "bfloat16" else 2e-3) + 2 * np.abs(want) * 2.0 ** (-7 if dtype == "bfloat16" else -10)
    assert not (err > tol).any(), f"{(err > tol).sum()} / {err.size} elements off, max err {err.max()}"
    if ctxs[0] == 1:                                             # a query without keys: a zero row, its neighbours unchanged
        z = run(np.concatenate([[0], ctx[1:]]).astype(np.int32))
        assert not z[0].any() and np.array_equal(z[1:], u[1:])
