"""bench.py on the GPU, on a 64-block config-2 batch: a plain run prints the
headline figure only and `--dump-outputs DIR` writes the last timed step's
output arrays (whole, or at bench.sample_positions) equal to the oracle's decode
of the same seeded batch; `--full` adds the roofline object, the CPU baseline
and the PCIe-inclusive pass to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from pebble_amd import _native as N
from pebble_amd.rowblk import gen_row_blocks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("roofline", "cpu_baseline", "e2e_pcie")


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--blocks", "64", *extra], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert all(k in d for k in HEADLINE) and d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    return d


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    import bench
    out = tmp_path / "out"
    d = run_bench("--dump-outputs", str(out))
    assert not set(EXTRAS) & set(d)
    buf, off, lens, n = gen_row_blocks(42, 64, 32768, 16, 16, 100)
    o = oracle.decode_batch(buf, off, lens, N.PBL_FMT_ROW)
    want = {"totals": np.array([o["n_kv"], o["key_bytes_total"], o["val_bytes_total"], o["n_restarts"], 0, 0],
                               np.uint64)}  # (status mask and bad blocks: none)
    sampled = 0
    for k in ("trailer", "kv_flags", "entry_off", "key_off", "val_off", "key_bytes", "val_bytes", "restarts",
              "blk_kv_base", "blk_key_base", "blk_val_base", "blk_rst_base", "blk_status"):
        x = o[k]
        if len(x) > bench.DUMP_SAMPLE:
            x = x[bench.sample_positions(len(x))]
            sampled += 1
        want[k] = x
    assert sampled >= 2  # (key and value bytes: the sampled form is covered)
    files = {}
    for k, x in want.items():
        if x.dtype.itemsize == 8:
            files[k + "_lo32"] = (x & np.uint64(0xFFFFFFFF)).astype(np.float64)
            files[k + "_hi32"] = (x >> np.uint64(32)).astype(np.float64)
        else:
            files[k] = x.astype(np.float32 if x.dtype.itemsize == 1 else np.float64)
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in files)
    for f, x in files.items():
        g = np.load(out / (f + ".npy"))
        assert g.dtype == x.dtype and np.array_equal(g, x), f
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64_000_000


def test_full_run_adds_the_extra_measurements():
    d = run_bench("--full", "--cpu-baseline-seconds", "0.2")
    assert all(k in d for k in EXTRAS)
    assert d["roofline"]["kernel_ms"] > 0 and d["cpu_baseline"]["value"] > 0 and d["e2e_pcie"]["value"] > 0
