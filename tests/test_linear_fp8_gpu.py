"""GPU tests (-m gpu) of the FP8 (e4m3) weight stream (kernels/linear_fp8.hip), both 16-bit builds: nvr_weight_quantize_fp8 against a numpy restatement
of its scale and byte rules (scales and dequantised weights exact), the three GEMM forms against float64 x @ Wd.T on the dequantised weights with the
bounds of test_decode_gemms_over_large_weights (same f32 MFMA accumulation, weights dequantise exactly), and the refusals."""
import functools

import numpy as np
import pytest

import nvr_import
from test_kv_fp8_gpu import E4M3, e4m3_encode, dev, dtype, to16  # noqa: F401  (dtype: the fixture that selects the build)

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu
WGS = 256                                                        # persistent workgroups of the GEMM grid


def quant_ref(W):
    """scales (2^e: the smallest e >= -15 with amax <= 448 * 2^e; all-zero row: e = 0) and dequantised weights of row-major 16-bit values W"""
    W = np.asarray(W, np.float64)
    am = np.abs(W).max(1)
    e = np.ceil(np.log2(np.where(am > 0, am, 448.0) / 448.0))
    e += am > 448.0 * 2.0 ** e                                   # (the logarithm may be off by one at a boundary)
    e -= am <= 448.0 * 2.0 ** (e - 1)
    sc = 2.0 ** np.where(am > 0, np.maximum(e, -15), 0)
    return sc.astype(np.float32), (E4M3[e4m3_encode(W / sc[:, None])].astype(np.float64) * sc[:, None]).astype(np.float32)


def from16(buf, shape, dtype):
    u = buf.to_numpy(shape, np.uint16)
    return (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)


def quantize(Wbits, N, K, dtype):
    d_q, d_s, d_d = nvr.DeviceBuffer(N * K), nvr.DeviceBuffer(N * 4), nvr.DeviceBuffer(N * K * 2)
    nvr.check(nvr.lib().nvr_weight_quantize_fp8(dev(Wbits).ptr, N, K, d_q.ptr, d_s.ptr, d_d.ptr, None))
    return d_q, d_s, from16(d_d, (N, K), dtype)


@pytest.mark.parametrize("N,K", [(16, 64), (48, 192)])
def test_weight_quantize_fp8_scales_and_dequantised_weights_exact(dtype, N, K):
    W = np.random.default_rng(5).standard_normal((N, K)) * 0.02
    W[0] = 0                                                     # e = 0
    W[1] = np.clip(W[1], -0.1, 0.1); W[1, 3] = -448 * 2.0 ** -12  # amax exactly 448 * 2^e
    W[2] *= 2.0 ** -8                                            # amax < 448 * 2^-16: the e = -15 clamp
    W[N - 1] *= 2.0 ** 6
    Wf, Wb = to16(W, dtype)
    _, d_s, Wd = quantize(Wb, N, K, dtype)
    sc, want = quant_ref(Wf)
    assert sc[0] == 1 and sc[1] == 2.0 ** -12 and sc[2] == 2.0 ** -15
    assert np.array_equal(d_s.to_numpy((N,), np.float32), sc) and np.array_equal(Wd, want)


@functools.lru_cache(maxsize=None)
def _case(dtype, K, rows):
    """16-bit weights 0.02 * normal, one row of every 16-row tile at another magnitude (a wrong row <-> scale pairing cannot pass), 64 rows of x"""
    rng = np.random.default_rng(K + rows)
    W = rng.standard_normal((rows, K)) * 0.02
    t = np.arange(rows // 16)
    W[t * 16 + (5 * t) % 16] *= np.where(t % 2, 2.0 ** -6, 2.0 ** 6)[:, None]
    return to16(W, dtype)[1], to16(rng.standard_normal((64, K + 24)), dtype)


def _close(got, want, ulps, dtype, what):
    err, tol = np.abs(got - want), 3e-4 + ulps * np.abs(want) * 2.0 ** (-7 if dtype == "bfloat16" else -10)
    print(f"{what}: max |err| {err.max():.3e}")
    assert not (err > tol).any(), f"{what}: {(err > tol).sum()} / {err.size} elements off, max err {err.max()}"


# T: one per MFMA column-tile count; K: one k-step, fewer k-steps than waves, several image chunks with a ragged last one; N: one tile, and one workgroup
# with two tiles; pad: row stride of x beyond K.  (64, 64, 16 * (3 * WGS + 1)): the SiLU form's second pass over K (3 tiles per pass at 64 rows)
@pytest.mark.parametrize("T,K,N,pad", [(1, 64, 16, 0), (17, 192, 16 * (WGS + 1), 8), (33, 2048 + 64, 16, 24), (64, 2048 + 64, 16 * (WGS + 1), 0),
                                       (64, 192, 16, 8), (1, 2048 + 64, 16 * (WGS + 1), 24), (17, 64, 16, 0), (33, 192, 16 * (WGS + 1), 0),
                                       (64, 64, 16 * (3 * WGS + 1), 0)])
def test_linear_fp8_plain_and_silu(dtype, T, K, N, pad):
    Wb, (xf, xb) = _case(dtype, K, 2 * N)
    d_q, d_s, Wd = quantize(Wb, 2 * N, K, dtype)
    ldx = K + pad
    x, d_x = xf[:T, :K].astype(np.float64), dev(np.ascontiguousarray(xb[:T, :ldx]))
    full = x @ Wd.astype(np.float64).T                           # [T, 2N]: rows 0..N-1 of W are also the plain form's weight
    d_y = nvr.DeviceBuffer(T * N * 2)
    nvr.check(nvr.lib().nvr_linear_fp8(d_x.ptr, ldx, d_q.ptr, d_s.ptr, T, K, N, d_y.ptr, None))
    _close(from16(d_y, (T, N), dtype), to16(full[:, :N], dtype)[0], 1, dtype, "plain")
    nvr.check(nvr.lib().nvr_linear_silu_mul_fp8(d_x.ptr, ldx, d_q.ptr, d_s.ptr, T, K, N, d_y.ptr, None))
    g, u = to16(full[:, :N], dtype)[0].astype(np.float64), to16(full[:, N:], dtype)[0].astype(np.float64)
    _close(from16(d_y, (T, N), dtype), to16(g / (1 + np.exp(-g)) * u, dtype)[0], 2, dtype, "silu")


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("T,N,pad", [(17, 16, 0), (64, 16 * (WGS + 1), 8)])
def test_linear_fp8_splitk_slabs(dtype, T, N, pad, S):
    K = 192
    Wb, (xf, xb) = _case(dtype, K, N)
    d_q, d_s, Wd = quantize(Wb, N, K, dtype)
    d_slabs = nvr.DeviceBuffer(S * T * N * 4)
    nvr.check(nvr.lib().nvr_linear_splitk_fp8(dev(np.ascontiguousarray(xb[:T, :K + pad])).ptr, K + pad, d_q.ptr, d_s.ptr, T, K, N, S, d_slabs.ptr, None))
    got, want = d_slabs.to_numpy((S, T, N), np.float32).astype(np.float64).sum(0), xf[:T, :K].astype(np.float64) @ Wd.astype(np.float64).T
    print(f"slabs S={S}: max |err| {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=6e-4)


@pytest.mark.parametrize("dtype,T,K,N,S", [("float16", 65, 192, 16, 1), ("bfloat16", 8, 96, 16, 1), ("float16", 8, 192, 24, 1), ("bfloat16", 8, 192, 16, 2),
                                           ("float32", 8, 192, 16, 1)], indirect=["dtype"])
def test_linear_fp8_refusals(dtype, T, K, N, S):
    """answered before anything is launched: NVR_ERR_UNSUPPORTED for the shapes and the float32 ops, NVR_ERR_INVALID_ARG for a null pointer"""
    b, l = dev(np.zeros(1 << 16, np.uint8)), nvr.lib()
    assert l.nvr_linear_splitk_fp8(b.ptr, K, b.ptr, b.ptr, T, K, N, S, b.ptr, None) == -10
    if S == 1:
        assert l.nvr_linear_fp8(b.ptr, K, b.ptr, b.ptr, T, K, N, b.ptr, None) == -10
        assert l.nvr_linear_silu_mul_fp8(b.ptr, K, b.ptr, b.ptr, T, K, N, b.ptr, None) == -10
        if (K, N) != (192, 16) or dtype == "float32":
            assert l.nvr_weight_quantize_fp8(b.ptr, N, K, b.ptr, b.ptr, None, None) == -10
    if dtype != "float32":
        assert l.nvr_linear_fp8(b.ptr, 192, None, b.ptr, 8, 192, 16, b.ptr, None) == -7
