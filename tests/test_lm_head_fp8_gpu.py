"""GPU test (-m gpu) of the LM head over FP8 (e4m3) weight bytes (kernels/lm_head_fp8.hip), in the shape of test_lm_head_logits_and_argmax_partials:
f32 logits against float64 x @ Wd.T on the dequantised weights (conversion and row scale are exact, only the f32 summation order differs: that test's
bound), the arg-max partials EXACTLY the lowest-index arg-max of the logits the kernel wrote, the same partials without logits, the refusals."""
import ctypes as C

import numpy as np
import pytest

import nvr_import
import oracle
from test_kv_fp8_gpu import dev, dtype, to16  # noqa: F401  (dtype: the fixture that selects the build)
from test_linear_fp8_gpu import quantize

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu
P = 2048                                                         # NVR_LM_HEAD_MAX_PARTS

# which path of the kernel a case reaches (resident: T <= 32 and K <= 2048, MT = ceil(T / 16) column tiles; chunked: 1024-column image chunks at MT = 2,
# 512-column ones at MT = 3 / 4; a tile's 64-column blocks go eight at a time, the rest one by one; 256 workgroups x 8 waves own the 16-row tiles)
CASES = [("float16", 1, 1024, 48),          # resident MT 1, 15 padded rows; 3 tiles on 8 waves: idle waves write neutral partials
         ("bfloat16", 1, 1024, 48),
         ("float16", 16, 320, 640),         # resident MT 1, no padded row; 5 blocks: only the one-by-one rest
         ("bfloat16", 17, 576, 2064),       # resident MT 2, padded rows; 9 blocks: a group and a rest; 129 tiles: a partly filled last workgroup
         ("float16", 32, 2048, 640),        # resident MT 2, the largest (128 KiB) image
         ("float16", 32, 4096, 2064),       # chunked at <= 32 rows, four chunks
         ("bfloat16", 32, 4096, 2064),
         ("float16", 1, 2112, 48),          # chunked at <= 16 rows (the MT 2 instance over one row), ragged last chunk (2 x 1024 + 64)
         ("float16", 33, 320, 48),          # chunked MT 3, one ragged chunk (K no multiple of 256), padded rows
         ("bfloat16", 49, 1088, 16 * 4099),  # chunked MT 4, padded rows, three chunks (ragged last); 4099 tiles on 2048 waves: 3 waves own 3 tiles, the others 2
         ("float16", 64, 1024, 2064)]       # chunked MT 4, every row live


@pytest.mark.parametrize("dtype,T,K,N", CASES, indirect=["dtype"])
def test_lm_head_fp8_logits_and_argmax_partials(dtype, T, K, N):
    rng = np.random.default_rng(31)
    W = rng.standard_normal((N, K), dtype=np.float32) * np.float32(0.05)
    W[N // 3] = W[5]; W[N - 1] = W[5]                            # identical rows quantise to identical bytes and scales: exact ties
    x = rng.standard_normal((T, K), dtype=np.float32)
    x[0] = W[5] * 8                                              # that tied logit is the row maximum of token 0
    (xf, xb), Wb = to16(x, dtype), to16(W, dtype)[1]
    d_q, d_s, Wd = quantize(Wb, N, K, dtype)
    d_x, d_y, l = dev(xb), nvr.DeviceBuffer(T * N * 4), nvr.lib()
    d_pv, d_pi, nparts = nvr.DeviceBuffer(P * T * 4), nvr.DeviceBuffer(P * T * 4), C.c_int32(0)
    nvr.check(l.nvr_lm_head_fp8(d_x.ptr, K, d_q.ptr, d_s.ptr, T, K, N, d_y.ptr, d_pv.ptr, d_pi.ptr, C.byref(nparts), None))
    assert 1 <= nparts.value <= P
    y, ref = d_y.to_numpy((T, N), np.float32), xf.astype(np.float64) @ Wd.astype(np.float64).T
    print(f"max |logit - float64| {np.abs(y - ref).max():.3e} (max |logit| {np.abs(ref).max():.2f})")
    np.testing.assert_allclose(y, ref, rtol=2e-5, atol=3e-4)
    d_tok, d_val = nvr.DeviceBuffer(T * 8), nvr.DeviceBuffer(T * 4)
    nvr.check(l.nvr_argmax_partials(d_pv.ptr, d_pi.ptr, nparts.value, T, d_tok.ptr, d_val.ptr, 1000, None))
    want = np.asarray([oracle.argmax(y[t]) for t in range(T)])
    assert (d_tok.to_numpy((T,), np.int64) - 1000).tolist() == want.tolist()
    assert np.array_equal(d_val.to_numpy((T,), np.float32), y[np.arange(T), want])
    assert want[0] == 5                                          # three-way tie at rows 5, N // 3, N - 1 -> lowest index
    # logits == NULL (what a greedy step asks for): the same partials, bit for bit
    d_pv2, d_pi2, np2 = nvr.DeviceBuffer(P * T * 4), nvr.DeviceBuffer(P * T * 4), C.c_int32(0)
    nvr.check(l.nvr_lm_head_fp8(d_x.ptr, K, d_q.ptr, d_s.ptr, T, K, N, None, d_pv2.ptr, d_pi2.ptr, C.byref(np2), None))
    n = nparts.value * T
    assert np2.value == nparts.value
    assert np.array_equal(d_pv2.to_numpy((P * T,), np.uint32)[:n], d_pv.to_numpy((P * T,), np.uint32)[:n])
    assert np.array_equal(d_pi2.to_numpy((P * T,), np.int32)[:n], d_pi.to_numpy((P * T,), np.int32)[:n])
    # refused, not approximated: N no multiple of 16, more than 64 rows, the float32 ops dtype
    args = (d_q.ptr, d_s.ptr), (d_y.ptr, d_pv.ptr, d_pi.ptr, C.byref(nparts), None)
    assert l.nvr_lm_head_fp8(d_x.ptr, K, *args[0], T, K, N - 8, *args[1]) == -10
    assert l.nvr_lm_head_fp8(d_x.ptr, K, *args[0], 65, K, N, *args[1]) == -10
    nvr.check(l.nvr_ops_set_dtype(b"float32"))                  # (the fixture restores float16)
    assert l.nvr_lm_head_fp8(d_x.ptr, K, *args[0], T, K, N, *args[1]) == -10
