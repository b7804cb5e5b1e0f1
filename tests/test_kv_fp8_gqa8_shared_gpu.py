"""GPU tests (-m gpu) of the shared-prefix decode attention over the FP8 (e4m3fn) KV cache at 8 query heads per kv head (nvr_paged_attn_decode_shared_fp8:
flash_shared_fp8_kernel<D, 8> + attn_fp8_mfma_kernel<D, 8, true>), both 16-bit builds, against oracle.attn_decode on the dequantised caches."""
import numpy as np
import pytest

import nvr_import
from test_kv_fp8_gpu import dtype, to16  # noqa: F401  (dtype: the fixture)
from test_kv_fp8_shared_gpu import _all, _call

nvr = nvr_import.load()
pytestmark = pytest.mark.gpu

CASES = [
    _all(5, 8, 1, 64, 64, 1, [0, 1, 63, 64, 130], (1.0, 1.0)),                              # members without own keys, partial blocks
    _all(2, 16, 2, 128, 256, 1, [0, 0], (1.0, 1.0)),                                        # only shared partitions exist
    _all(35, 16, 2, 128, 128, 2, np.random.default_rng(1).integers(0, 300, 35), (0.25, 4.0)),   # two full 16-row tiles and a ragged third, several shared partitions, scales
    _all(3, 8, 1, 128, 64, 1, [700, 257, 0], (1.0, 1.0)),                                   # several own partitions of more than four steps, an empty one
    _all(4, 8, 1, 64, 64, 65, [3, 0, 64, 17], (1.0, 1.0)),                                  # more than 64 shared block-table entries
    # a group of 6 inside a batch of 9: kv0_rows, non-members (contexts 1, 123, 198) on blocks of their own
    (9, 8, 1, 128, 64, 2, (1, 137, 128, 123, 192, 259, 198, 129, 168), (1, 2, 4, 5, 7, 8), (0.5, 2.0)),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-H{c[1]}-KVH{c[2]}-D{c[3]}-bs{c[4]}-P{c[5]}" for c in CASES])
def test_fp8_gqa8_paged_attn_decode_shared_prefix(dtype, case):
    """measured max |err| (MI355X): fp16 4.9e-4, bf16 2.0e-3 over all cases"""
    B, H, D = case[0], case[1], case[3]
    rc, d_out, ref = _call(dtype, case)
    nvr.check(rc)
    u, want = d_out.to_numpy((B, H, D), np.uint16), to16(ref, dtype)[0]
    got = (u.astype(np.uint32) << 16).view(np.float32) if dtype == "bfloat16" else u.view(np.float16).astype(np.float32)
    err = np.abs(got - want)
    print(f"max |err| {err.max():.3e}")
    # test_fp8_paged_attn_decode_shared_prefix's bound: the rounding points are the same kernels'
    tol = (1.6e-2 + 2 * np.abs(want) * 2.0 ** -7) if dtype == "bfloat16" else (2e-3 + 2 * np.abs(want) * 2.0 ** -10)
    assert np.isfinite(got).all(), "a NaN byte behind a context reached the output"
    assert not (err > tol).any(), f"{(err > tol).sum()} / {err.size} elements off, max err {err.max()}"
