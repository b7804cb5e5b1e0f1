"""bench.py's in-run counter passes (roofline.traffic, prefill.mfma_busy_frac_pmc): the parsing of rocprofv3's counter table is pure and is
checked here on synthetic tables; the passes themselves run on the GPU box inside the bench."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("nvr_bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _rows(kernel, counter, values, first_id=1):
    return [{"Dispatch_Id": str(first_id + i), "Kernel_Name": kernel, "Counter_Name": counter, "Counter_Value": str(v)} for i, v in enumerate(values)]


def test_attention_traffic_is_bytes_over_algorithmic_bytes_of_the_pass():
    m = bench.MODELS["qwen3-0.6b"]
    sh, B, P = m["shape"], m["batch"], m["prompt_len"]
    steps, warm = 6, 2
    n, L = steps + warm, sh["layers"]
    ctxs = [P + i for i in range(1, n + 1) for _ in range(L)] + [P + n + 1] * (2 * L)
    alg = lambda c: B * c * sh["kvh"] * sh["d"] * 2 * 2 + 2 * B * sh["h"] * sh["d"] * 2
    # a kernel that fetches exactly its algorithmic bytes: FETCH_SIZE is in KiB and counts half of them on gfx950
    rows = _rows("void nvr::k::attn_rows_kernel<128, 2, ...>(AttnParams)", "FETCH_SIZE", [alg(c) / 2048.0 for c in ctxs])
    rows += _rows("some_other_kernel", "FETCH_SIZE", [1e9] * 5, first_id=1000)
    got = bench.attention_traffic_from_rows(rows, "qwen3-0.6b", steps, warm)
    assert got["dispatches"] == L * (n + 2) and abs(got["traffic_over_algorithmic"] - 1.0) < 2e-4, got
    assert abs(got["mean_context"] - sum(ctxs) / len(ctxs)) < 0.01
    # 7 % over-fetch shows up as 1.07; a pass with the wrong number of dispatches is refused with a reason
    over = bench.attention_traffic_from_rows([dict(r, Counter_Value=str(float(r["Counter_Value"]) * 1.07)) for r in rows], "qwen3-0.6b", steps, warm)
    assert abs(over["traffic_over_algorithmic"] - 1.07) < 1e-3
    assert isinstance(bench.attention_traffic_from_rows(rows[:-20], "qwen3-0.6b", steps, warm), str)
    # the live timing as a replayed graph adds one more sweep at the final context
    more = _rows("void nvr::k::attn_rows_kernel<128, 2, ...>(AttnParams)", "FETCH_SIZE", [alg(P + n + 1) / 2048.0] * L, first_id=5000)
    got3 = bench.attention_traffic_from_rows(rows + more, "qwen3-0.6b", steps, warm)
    assert got3["dispatches"] == L * (n + 3) and abs(got3["traffic_over_algorithmic"] - 1.0) < 2e-4, got3


def test_prefill_busy_share_takes_the_last_prefill_step_only():
    rows = []
    did = [0]

    def disp(kernel, busy, grbm):
        did[0] += 1
        for c, v in (("SQ_VALU_MFMA_BUSY_CYCLES", busy), ("GRBM_GUI_ACTIVE", grbm)):
            rows.append({"Dispatch_Id": str(did[0]), "Kernel_Name": kernel, "Counter_Name": c, "Counter_Value": str(v)})
    for rep in range(2):                                   # warm-up prefill, then the measured one: only the second counts
        disp("embedding_kernel", 0, 8 * 1000)
        for l in range(3):
            scale = 1 if rep else 5                        # (the warm-up has other numbers)
            disp("gemm256_kernelILi3ELi128E", 1024 * 400 * scale, 8 * 1000)      # 40 % busy
            disp("flash_prefill_kernel<128, 2>", 1024 * 300 * scale, 8 * 1000)   # 30 %
            disp("gemm256_kernelILi1ELi0E", 1024 * 500 * scale, 8 * 1000)        # 50 %
            disp("rmsnorm_kernel", 0, 8 * 100)
    disp("embed_rmsnorm_kernel", 0, 8 * 10)                # first decode step: ends the prefill step
    disp("gemm256_kernelILi1ELi0E", 1024 * 999, 8 * 1000)
    got = bench.prefill_busy_from_rows(rows)
    assert got["per_kernel"]["qkv+RoPE+store"] == 0.4 and got["per_kernel"]["flash_prefill"] == 0.3 and got["per_kernel"]["o / down + residual"] == 0.5
    busy = 3 * (400 + 300 + 500) * 1024; cyc = 1000 + 3 * (3 * 1000 + 100)
    assert abs(got["step_weighted"] - busy / (1024 * cyc)) < 1e-3 and got["dispatches"] == 1 + 3 * 4


@pytest.mark.gpu
def test_plain_run_times_the_given_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` makes the headline measurement only (no side block, `roofline` null), reports the K it was
    given and a positive ms_per_step, and with --dump-outputs writes the last timed step's tokens and logits: same arguments, same arrays."""
    dumps = []
    for i in range(2):
        d = tmp_path / f"dump{i}"
        cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d)],
                            check=True, stdout=subprocess.PIPE, text=True, timeout=300, cwd=str(tmp_path))
        line = json.loads([l for l in cp.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "tokens/s" and line["higher_is_better"] is True
        assert abs(line["value"] - bench.MODELS["qwen3-0.6b"]["batch"] / line["ms_per_step"] * 1e3) < 1e-2 * line["value"]
        assert line["roofline"] is None and not {"cpu_baseline", "configs3", "batch_sweep", "prefill_sweep", "roofline_chain", "bf16", "float32_path"} & set(line)
        assert sorted(os.listdir(d)) == ["logits.npy", "tokens.npy"]
        dumps.append({n: np.load(d / n) for n in os.listdir(d)})
    B, V = bench.MODELS["qwen3-0.6b"]["batch"], 151936
    a, b = dumps
    assert a["tokens.npy"].dtype == np.float64 and a["tokens.npy"].shape == (B,) and a["logits.npy"].dtype == np.float32 and a["logits.npy"].shape == (B, V)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20 and np.isfinite(a["logits.npy"]).all()
    assert np.array_equal(a["logits.npy"].argmax(1), a["tokens.npy"].astype(np.int64))           # greedy: the tokens are the arg-max of the dumped logits
    assert all(np.array_equal(a[n], b[n]) for n in a)
