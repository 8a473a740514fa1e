#!/usr/bin/env python3
"""Benchmark: raw-block GiB/s decoded to KV arrays (device-resident).

One "step" = one decode pass of the hot path over one batch of synthetic data
blocks already resident in HBM.  Default workload (`--workload row`) is
BASELINE.json config 2 per GPU: 64 Ki x 32 KiB row-format blocks, restart
interval 16, 16 B user keys / 100 B values.  `--workload col` is config 3
(64 Ki x 32 KiB colblk blocks, cockroachkvs crdb1 schema, 22 B keys / 128 B
values); `--workload mixed` is config 4's per-GPU shard (128 Ki blocks, even
ids row / odd ids colblk, 1 Mi blocks over 8 GPUs); `--workload zipf` is
config 5 per GPU (64 Ki variable-length blocks targeting 32 KiB, Zipf(1.1) key
lengths 8-1024 B and value lengths 0-64 KiB, `--restart-interval` 1/16/32,
`--zipf-format row|col`); `--workload transform` times pbl_transform_batch
(SyntheticSeqNum + HideObsoletePoints + a 12-byte SyntheticPrefix) over
config 2 already decoded in HBM.  With
N > 1 (torch.distributed.run, one rank per GPU, RCCL) every rank decodes its own
64 Ki-block shard (weak scaling) and each step also performs the offset concat:
an all-gather of per-rank totals and the rebase of the per-block bases.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the steps
and prints the headline figure (`value`, `ms_per_step`) with the workload's
description.  `--dump-outputs DIR` also writes what the last timed step left in
the output arrays as DIR/<name>.npy (see dump_outputs).  `--full` adds the
extra objects, each a measurement or a check of its own: `roofline` (dominant
kernel, HBM bound, algorithmic bytes / live HIP-event kernel time; the whole
output copied back and its totals checked), `cpu_baseline` (the oracle's
C restatement of rowblk.Iter timed on this host's cores on a bounded sample;
reported, not the target) and `e2e_pcie` (the PCIe-inclusive pipeline).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

METRIC = "raw-block GiB/s decoded to KV arrays (device-resident), 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)



def lib_sha16() -> str:
    """sha256[:16] of the decoder library this process loads (PBL_LIB or the
    in-tree build): a traffic file counts only for the build it measured."""
    import hashlib
    from pebble_amd import _native as N
    with open(N.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]

def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--workload", choices=["row", "col", "mixed", "zipf", "rowmix", "transform", "cfg1"], default="row")
    p.add_argument("--mix", choices=["zipf10", "tail8"], default="zipf10",
                   help="rowmix: config-2 blocks with every 10th a Zipf block, or every 8th a short tail block")
    p.add_argument("--blocks", type=int, default=0, help="blocks per GPU (0 = the workload's config)")
    p.add_argument("--block-size", type=int, default=32768)
    p.add_argument("--restart-interval", type=int, default=16)
    p.add_argument("--key-len", type=int, default=16)
    p.add_argument("--val-len", type=int, default=100)
    p.add_argument("--value-prefix", action="store_true")
    p.add_argument("--hide", type=int, default=0,
                   help="HideObsoletePoints fused (PBL_ROW_HIDE_OBSOLETE) on row / col batches whose every N-th "
                        "KV per block is an obsolete point (0: off)"),
    p.add_argument("--tiering", type=int, default=0,
                   help="col workload: Pebblev8 blocks with the tiering columns (span ids 1..N), decoded with "
                        "PBL_COL_TIERING into the per-KV KVMeta arrays (0: off)")
    p.add_argument("--zipf-format", choices=["row", "col"], default="row",
                   help="config 5 block format (col = colblk DefaultKeySchema)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--full", action="store_true",
                   help="also the roofline object (whole output copied back and checked), the CPU baseline and the "
                        "PCIe-inclusive pass; a plain run only times the steps")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the output arrays of the last step as DIR/<name>.npy "
                        "(float32 / float64; a fixed seeded sample of the long ones)")
    p.add_argument("--cpu-baseline-seconds", type=float, default=10.0)
    p.add_argument("--cpu-threads", type=int, default=0,
                   help="CPU-baseline threads (0 = the CPUs this process may run on, capped at the box's CPU "
                        "share OMP_NUM_THREADS when that is set)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    p.add_argument("--no-e2e", action="store_true",
                   help="--full without the host->device->host (PCIe-inclusive) pass")
    p.add_argument("--e2e-chunk", type=int, default=2048, help="blocks per PCIe pipeline chunk")
    p.add_argument("--kernel", choices=["auto", "single", "pipe", "pool"], default="auto",
                   help="A/B: colblk batches single / pipe "
                        "(PBL_KERNEL_SINGLE / PBL_KERNEL_PIPE)")
    p.add_argument("--launch-check", action="store_true",
                   help="launcher self-test without a GPU: N gloo ranks report in, rank 0 prints one JSON line")
    p.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                   help="torch.distributed backend for N > 1 (nccl = RCCL over xGMI; gloo = CPU rehearsal)")
    return p.parse_args()


def self_launch(a) -> int:
    """`--gpus N` with N > 1 and no torch.distributed.run around us: start N
    ranks (one per GPU) through torch.distributed.run as a CHILD process and
    return its exit code.  Nothing in this parent touches the GPU (no exec
    from a process that has initialised it)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", env.get("OMP_NUM_THREADS", "16"))
    return subprocess.run(cmd, env=env).returncode


def launch_check(a) -> None:
    """The rank plumbing of main() on gloo (CPU): every rank reports
    (rank, local rank, world); rank 0 prints one JSON line."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        dist.init_process_group("gloo")
        mine = torch.tensor([rank, local, world], dtype=torch.int64)
        parts = [torch.zeros(3, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(parts, mine)
        seen = [p.tolist() for p in parts]
    else:
        seen = [[0, 0, 1]]
    if rank == 0:
        print(json.dumps({"metric": METRIC, "launch_check": True, "n_gpus": world, "ranks": seen,
                          "parallelism": f"shard{world}" + ("+rccl_offset_concat" if world > 1 else "")}),
              flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def cpu_threads(a) -> tuple:
    """(threads used, CPUs visible): the CPUs this process may run on, capped at
    the box's CPU share (OMP_NUM_THREADS) when the environment sets one."""
    visible = len(os.sched_getaffinity(0))
    if a.cpu_threads:
        return a.cpu_threads, visible
    share = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return (min(visible, share) if share > 0 else visible), visible


def alg_bytes(h: dict, nb: int, input_bytes: int) -> int:
    """Algorithmic bytes of one decode launch: every input
    byte read once plus every output byte written once."""
    n = h["n_kv"]
    out = (8 * n            # trailer
           + (16 * n if "tiering_span_id" in h else 0)  # KVMeta (span, attribute)
           + n              # kv_flags
           + 4 * n          # entry_off
           + 2 * 4 * (n + nb)  # key_off, val_off (N+1 per block)
           + h["key_bytes_total"] + h["val_bytes_total"]
           + 4 * h["n_restarts"]
           + 4 * 8 * (nb + 1)  # blk_{kv,key,val,rst}_base
           + 4 * nb)        # blk_status
    return input_bytes + 12 * nb + out


def concat_step(dist, gathered, local_totals, rebase) -> None:
    """The offset concat of one step: all-gather every rank's
    4 totals {n_kv, key bytes, value bytes, restarts} and rebase this rank's
    per-block bases by the exclusive prefix of the lower ranks."""
    dist.all_gather_into_tensor(gathered, local_totals)
    rebase(gathered)


def plumbing(a, world, rank, dist) -> None:
    """No GPU here (`--dist-backend gloo` rehearsal on CPU): the rank, timing
    and offset-concat plumbing of main() on a small synthetic row batch.  The
    decode itself needs the device, so each step restores the per-block bases a
    decode would leave (block-relative exclusive scans of the blocks' restart
    counts and lengths: any per-block aggregate exercises the rebase), then runs
    concat_step -- the same all-gather + rebase as the GPU step, the rebase as a
    CPU-tensor add of shard.exclusive_bases.  Rank 0 prints one JSON line with
    the concat checked against every rank's totals."""
    import copy
    from pebble_amd import _native as N
    from pebble_amd.shard import exclusive_bases
    ar = copy.copy(a)
    ar.workload = "row" if a.workload not in ("row", "zipf") else a.workload
    # this rank's byte-balanced shard of one global batch, as main() cuts it
    (buf, off, lens, n_kv, _), shard, rank_bytes = global_shard(ar, world, rank, dist, None, a.blocks or 64, N)
    nb = len(off)
    nres = np.array([int.from_bytes(buf[int(o) + int(l) - 4: int(o) + int(l)].tobytes(), "little")
                     for o, l in zip(off, lens)], np.int64)
    per = np.stack([nres, lens.astype(np.int64), lens.astype(np.int64) // 2, nres])  # [4, nb]
    local = torch.from_numpy(np.concatenate([np.zeros((4, 1), np.int64), np.cumsum(per, 1)], 1))  # [4, nb+1]
    totals = local[:, -1].contiguous()
    bases = local.clone()
    gathered = torch.zeros(world * 4, dtype=torch.int64)

    def step():
        bases.copy_(local)  # what the decode writes: this rank's own exclusive scan
        if world > 1:
            concat_step(dist, gathered, totals, lambda g: bases.add_(exclusive_bases(g, rank).view(4, 1)))

    for _ in range(a.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        firsts = torch.zeros(world * 4, dtype=torch.int64)
        dist.all_gather_into_tensor(firsts, bases[:, 0].contiguous())
        tot = gathered.view(world, 4)
        ok = all(torch.equal(firsts.view(world, 4)[r], tot[:r].sum(0)) for r in range(world))
    else:
        ok = True
    if a.dump_outputs and rank == 0:  # (no decode here: the rebased per-block bases are the step's output)
        os.makedirs(a.dump_outputs, exist_ok=True)
        np.save(os.path.join(a.dump_outputs, "blk_bases.npy"), bases.numpy().astype(np.float64))
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": None, "unit": "GiB/s", "n_gpus": world, "steps": a.steps,
                          "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 4),
                          "plumbing": True, "dist_backend": a.dist_backend, "concat_ok": bool(ok),
                          "note": "no GPU: decode not run; rank, timing and offset-concat plumbing only",
                          "config": {"workload": f"{ar.workload} blocks, byte-balanced shards of one global batch "
                                                 f"(plumbing)",
                                     "global_batch_blocks": int(shard[2]), "shard_blocks": [int(shard[0]), int(shard[1])],
                                     "input_bytes_per_rank": [int(x) for x in rank_bytes],
                                     "parallelism": f"shard{world}" + ("+offset_concat" if world > 1 else "")}}),
              flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def workload_info(a, nb, N):
    """(format, dominant kernel name, workload description) of a.workload."""
    row_kernel = "rowblk_pool_kernel"
    if a.workload in ("row", "transform"):
        kernel = "tf_count_kernel+tf_scan_kernel+tf_scatter_kernel" if a.workload == "transform" else row_kernel
        wl = ("transform pass (SyntheticSeqNum, HideObsoletePoints, 12 B SyntheticPrefix) over " if a.workload ==
              "transform" else "") + (f"config2: {nb} x {a.block_size // 1024} KiB row-format blocks per GPU, restart interval "
              f"{a.restart_interval}, {a.key_len} B keys / {a.val_len} B values" + (", value prefix" if a.value_prefix else "")
              + (f", every {a.hide}th KV obsolete, HideObsoletePoints fused" if a.hide else ""))
        return N.PBL_FMT_ROW, kernel, wl
    if a.workload == "rowmix":
        return N.PBL_FMT_ROW, row_kernel, (
            f"row-shape mix: {nb} row blocks per GPU, config-2 blocks with " +
            ("every 10th a config-5 Zipf block (restart interval 16)" if a.mix == "zipf10" else
             "every 8th a short table-tail block (2 / 4 / 8 KiB)"))
    if a.workload == "col":
        kernel = ("colblk_decode_kernel" if a.kernel == "single" and not a.hide else
                  "colblk_pipe_kernel" if a.hide or a.kernel == "pipe" else
                  "colblk_wave_size_kernel+bases_scan_kernel+colblk_wave_emit_kernel")
        return N.PBL_FMT_COL_CRDB1, kernel, (
            f"config3: {nb} x {a.block_size // 1024} KiB colblk blocks per GPU, cockroachkvs crdb1 schema "
            f"(KeyGenConfig alphabet 26, RoachKeyLen 12, PrefixLenShared 4, 1 key/prefix), 128 B values"
            + (f", every {a.hide}th row isObsolete, HideObsoletePoints fused" if a.hide else "")
            + (f", Pebblev8 tiering columns (span ids 1..{a.tiering}) decoded to per-KV KVMeta" if a.tiering else ""))
    if a.workload == "zipf":
        fmt = N.PBL_FMT_ROW if a.zipf_format == "row" else N.PBL_FMT_COL_DEFAULT
        kernel = (("row_wave_size_kernel+bases_scan_kernel+row_wave_emit_kernel" if a.kernel != "pool" else row_kernel)
                  if fmt == N.PBL_FMT_ROW else "colblk_decode_kernel" if a.kernel == "single" else "colblk_pipe_kernel" if a.kernel == "pipe"
                  else "colblk_wave_size_kernel+bases_scan_kernel+colblk_wave_emit_kernel")
        return fmt, kernel, (f"config5: {nb} variable-length blocks per GPU targeting {a.block_size // 1024} KiB, "
                             + (f"row format, restart interval {a.restart_interval}" if fmt == N.PBL_FMT_ROW
                                else "colblk DefaultKeySchema")
                             + ", Zipf(1.1) key lengths 8-1024 B / value lengths 0-64 KiB")
    # (the sequential mixed path: split + colblk size pass + the row
    # staging-pool kernel over the row ids + colblk pipeline, timed together)
    return N.PBL_FMT_ROW, ("colblk_wave_size_kernel+rowblk_pool_kernel+" +
                           ("mixed_col_kernel" if a.hide else "colblk_wave_emit_kernel")), (
        f"config4 shard: {nb} x {a.block_size // 1024} KiB blocks per GPU, even ids row-format "
        f"(config-2 shape), odd ids colblk crdb1 (config-3 shape)")


def gen_range(a, first: int, n: int, N):
    """Global blocks [first, first + n) of the workload's batch (seed a.seed):
    (buf, off, lens, n_kv, block_fmt)."""
    from pebble_amd.colblk import gen_col_blocks
    from pebble_amd.rowblk import gen_row_blocks
    if a.workload in ("row", "transform"):
        return (*gen_row_blocks(a.seed, n, a.block_size, a.restart_interval, a.key_len, a.val_len, a.value_prefix,
                                n_threads=16, obsolete_every=a.hide, first_block=first), None)
    if a.workload == "rowmix":
        from pebble_amd.batch import gen_row_mix
        assert first == 0, "rowmix is a single-GPU workload"
        return (*gen_row_mix(a.seed, n, a.mix, n_threads=16), None)
    if a.workload == "col":
        return (*gen_col_blocks(a.seed, n, a.block_size, n_threads=16, obsolete_every=a.hide, tiering=a.tiering,
                                first_block=first), None)
    if a.workload == "zipf":
        from pebble_amd.batch import gen_zipf_blocks
        fmt = N.PBL_FMT_ROW if a.zipf_format == "row" else N.PBL_FMT_COL_DEFAULT
        return (*gen_zipf_blocks(a.seed, n, fmt, a.restart_interval, a.block_size, n_threads=16, first_block=first),
                None)
    # mixed (config 4): global block g is row block g // 2 (g even) or colblk
    # block g // 2 (g odd), at a fixed stride
    r0, r1 = (first + 1) // 2, (first + n + 1) // 2
    c0, c1 = first // 2, (first + n) // 2
    rb, ro, rl, rn = gen_row_blocks(a.seed, r1 - r0, a.block_size, a.restart_interval, a.key_len, a.val_len,
                                    a.value_prefix, n_threads=16, first_block=r0)
    cb, co, cl, cn = gen_col_blocks(a.seed, c1 - c0, a.block_size, n_threads=16, first_block=c0)
    g = first + np.arange(n)
    is_row = (g & 1) == 0
    ri, ci = g // 2 - r0, g // 2 - c0
    buf = np.zeros(n * a.block_size + 16, np.uint8)
    v = buf[: n * a.block_size].reshape(n, a.block_size)
    v[is_row] = rb[: (r1 - r0) * a.block_size].reshape(r1 - r0, a.block_size)[ri[is_row]]
    v[~is_row] = cb[: (c1 - c0) * a.block_size].reshape(c1 - c0, a.block_size)[ci[~is_row]]
    del rb, cb
    off = np.arange(n, dtype=np.uint64) * a.block_size
    lens = np.where(is_row, rl[np.clip(ri, 0, max(r1 - r0 - 1, 0))] if r1 > r0 else 0,
                    cl[np.clip(ci, 0, max(c1 - c0 - 1, 0))] if c1 > c0 else 0).astype(np.uint32)
    block_fmt = np.where(is_row, N.PBL_FMT_ROW, N.PBL_FMT_COL_CRDB1).astype(np.uint8)
    return buf, off, lens, rn + cn, block_fmt


def gather_ints(dist, dev, vals, world: int, backend: str) -> np.ndarray:
    """All-gather an int64 vector of the same length from every rank -> [world, n]."""
    t = torch.as_tensor(np.asarray(vals, np.int64))
    if backend == "nccl":
        t = t.to(dev)
        out = torch.empty(world * t.numel(), dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(out, t)
    else:
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        out = torch.cat(parts)
    return out.cpu().numpy().reshape(world, -1)


def global_shard(a, world, rank, dist, dev, nb, N):
    """This rank's byte-balanced shard of the global batch of world x nb
    blocks: ((buf, off, lens, n_kv, block_fmt), (start, end, global blocks),
    input bytes of every rank)."""
    if world == 1:
        g = gen_range(a, 0, nb, N)
        return g, (0, nb, nb), [int(g[2].astype(np.int64).sum())]
    from pebble_amd.shard import partition_blocks
    g = gen_range(a, rank * nb, nb, N)
    lens_all = gather_ints(dist, dev, g[2].astype(np.int64), world, a.dist_backend).reshape(-1)
    s, e = partition_blocks(lens_all, world)[rank]
    if (s, e) != (rank * nb, (rank + 1) * nb):
        del g
        g = gen_range(a, s, e - s, N)
    rank_bytes = gather_ints(dist, dev, [int(g[2].astype(np.int64).sum())], world, a.dist_backend).reshape(-1)
    return g, (s, e, world * nb), [int(x) for x in rank_bytes]


DUMP_SAMPLE = 1 << 18  # elements kept of a longer array: a dump stays under 64 MB whatever the batch


def _dump_array(dirname: str, name: str, x: np.ndarray) -> int:
    """DIR/<name>.npy, exact in a float type: 8-bit values as float32, 32-bit
    ones as float64, 64-bit ones as float64 halves <name>_lo32 / <name>_hi32."""
    if x.dtype.itemsize == 8:
        u = x.view(np.uint64)
        return (_dump_array(dirname, name + "_lo32", (u & np.uint64(0xFFFFFFFF)).astype(np.uint32))
                + _dump_array(dirname, name + "_hi32", (u >> np.uint64(32)).astype(np.uint32)))
    f = x.astype(np.float32 if x.dtype.itemsize == 1 else np.float64)
    np.save(os.path.join(dirname, name + ".npy"), f)
    return f.nbytes


def sample_positions(k: int) -> np.ndarray:
    """The sorted positions a dump keeps of an array of k > DUMP_SAMPLE elements."""
    return np.sort(np.random.default_rng(20240607).integers(0, k, DUMP_SAMPLE))


def dump_outputs(out, dirname: str) -> None:
    """--dump-outputs: the arrays a caller of the timed path receives (the
    DecodedBatch that decode_into / TransformPlan.launch filled in the last
    timed step), each cut to the length its totals give, as DIR/<name>.npy.
    An array longer than DUMP_SAMPLE is written as its elements at
    sample_positions(length) (gathered on the device): positions drawn by a
    fixed-seed generator from the length alone, so two builds that decode the
    same batch write the same positions."""
    os.makedirs(dirname, exist_ok=True)
    t = out.read_totals()
    nb, n = out.n_blocks, int(t.n_kv)
    arrays = [("trailer", out.trailer, n), ("kv_flags", out.kv_flags, n), ("entry_off", out.entry_off, n),
              ("key_off", out.key_off, n + nb), ("val_off", out.val_off, n + nb),
              ("key_bytes", out.key_bytes, int(t.key_bytes)), ("val_bytes", out.val_bytes, int(t.val_bytes)),
              ("restarts", out.restarts, int(t.n_restarts)),
              ("blk_kv_base", out.blk_kv_base, nb + 1), ("blk_key_base", out.blk_key_base, nb + 1),
              ("blk_val_base", out.blk_val_base, nb + 1), ("blk_rst_base", out.blk_rst_base, nb + 1),
              ("blk_status", out.blk_status, nb),
              ("tiering_span_id", out.tiering_span_id, n), ("tiering_attr", out.tiering_attr, n)]
    total = _dump_array(dirname, "totals", np.array(
        [t.n_kv, t.key_bytes, t.val_bytes, t.n_restarts, t.status_mask, t.n_bad_blocks], np.uint64))
    for name, x, k in arrays:
        if x is None:
            continue
        x = x[:k]
        if k > DUMP_SAMPLE:
            x = x[torch.from_numpy(sample_positions(k)).to(x.device)]
        total += _dump_array(dirname, name, x.cpu().numpy())
    assert total <= 64_000_000, total


def roofline(a, kernel, nb, input_bytes, kern_ms, hres, h_in=None) -> dict:
    """The `roofline` object of a --full line: algorithmic bytes of one launch
    (from the decoded arrays `hres`; `h_in`: the transform pass's input) over the
    HIP-event kernel time, and the measured HBM traffic where profiles/ holds
    it for this workload, kernel and build of the library."""
    ab = alg_bytes(hres, nb, input_bytes)
    if h_in is not None:  # the decoded arrays read once, the transformed ones written once
        ab = alg_bytes(h_in, nb, 0) + alg_bytes(hres, nb, 0) - 24 * nb
    achieved = ab / (kern_ms * 1e-3) / 1e9
    traffic = None
    tname = ("pmc_traffic" if a.workload == "row" and a.kernel == "auto" else
             f"pmc_traffic_{a.kernel}" if a.workload == "row" else
             f"pmc_traffic_zipf_ri{a.restart_interval}" if a.workload == "zipf" and a.zipf_format == "row" else
             f"pmc_traffic_{a.workload}") + (f"_hide{a.hide}" if a.hide else "") + (
             f"_tier{a.tiering}" if a.tiering else "") + ".json"
    tp = os.path.join(ROOT, "profiles", tname)
    if os.path.exists(tp):
        try:
            with open(tp) as f:
                pt = json.load(f)
            same_zipf = a.workload != "zipf" or (pt.get("restart_interval") == a.restart_interval
                                                  and pt.get("zipf_format") == a.zipf_format)
            # the PMC of THIS decode's kernels only (a file names the kernel(s) it measured)
            # ... and of THIS build of the library (the file records the sha256 of
            # the .so it was measured on)
            if (pt.get("workload_blocks") == nb and pt.get("block_size") == a.block_size
                    and pt.get("workload", "row") == a.workload and same_zipf and pt.get("kernel") == kernel
                    and pt.get("lib_sha16") == lib_sha16()):
                traffic = pt.get("hbm_bytes_per_launch")
        except Exception:
            traffic = None
    return {"bound": "hbm", "kernel": kernel, "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic, "alg_bytes_per_launch": ab, "kernel_ms": round(kern_ms, 4),
            "lib_sha16": lib_sha16(), "traffic_source": f"profiles/{tname}" if traffic else None,
            "input_GiB_per_s_kernel": round(input_bytes / (kern_ms * 1e-3) / 2**30, 1)}


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))
    if a.launch_check:
        launch_check(a)
        return
    if a.workload == "cfg1":
        config1(a)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if not torch.cuda.is_available():
        if world > 1:
            import torch.distributed as dist  # noqa: F811
            dist.init_process_group("gloo")
        plumbing(a, world, rank, dist)
        return
    if world > 1:
        import torch.distributed as dist  # noqa: F811
        torch.cuda.set_device(local)
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    from pebble_amd import _native as N
    from pebble_amd.batch import BlockBatch, Capacity, DecodedBatch, decode, decode_into, offset_concat
    from pebble_amd.colblk import gen_col_blocks
    from pebble_amd.rowblk import gen_row_blocks

    nb = a.blocks or (131072 if a.workload == "mixed" else 65536)
    flags = N.PBL_ROW_VALUE_PREFIX if a.value_prefix else 0
    if a.hide:
        flags |= N.PBL_ROW_HIDE_OBSOLETE
    meta = a.tiering > 0
    if meta:
        assert a.workload == "col", "--tiering applies to the col workload"
        flags |= N.PBL_COL_TIERING
    flags |= {"auto": 0, "single": N.PBL_KERNEL_SINGLE, "pipe": N.PBL_KERNEL_PIPE, "pool": N.PBL_KERNEL_POOL}[a.kernel]
    t0 = time.time()
    fmt, kernel, wl = workload_info(a, nb, N)
    # ONE global batch of world x nb blocks (block content = f(seed, global
    # index)), cut into contiguous byte-balanced ranges:
    # every rank generates its nominal range, the ranges' lengths are
    # all-gathered, shard.partition_blocks picks this rank's range, and the
    # blocks it lacks are generated (configs 2-4: the nominal ranges; config 5:
    # boundaries move to balance bytes)
    (buf, off, lens, n_kv, block_fmt), shard_range, rank_bytes = global_shard(a, world, rank, dist, dev, nb, N)
    nb = len(off)
    gen_s = time.time() - t0
    input_bytes = int(lens.astype(np.int64).sum())
    batch = BlockBatch.from_host(buf, off, lens, dev, fmt, flags, block_format=block_fmt)

    # size the outputs exactly with one decode, then reuse them every step
    first = decode(batch, meta=meta)
    t = first.read_totals()
    if a.hide:  # the visible KVs only: fewer than were written
        assert 0 < t.n_kv < n_kv and t.status_mask == 0, (t.n_kv, n_kv, t.status_mask)
        n_kv = int(t.n_kv)
    assert t.n_kv == n_kv and t.status_mask == 0, (t.n_kv, n_kv, t.status_mask)
    cap = Capacity(kv=int(t.n_kv), key=int(t.key_bytes), val=int(t.val_bytes), rst=int(t.n_restarts))
    stream = torch.cuda.current_stream(dev)
    plan = None
    if a.workload == "transform":
        # the decoded config-2 batch stays resident; each step transforms it
        from pebble_amd.transforms import TransformPlan, Transforms
        plan = TransformPlan(first, Transforms(synthetic_seq_num=12345, hide_obsolete_points=True,
                                               synthetic_prefix=b"tenant-0042/"), stream)
        out = plan.out
        h_in = first.to_host() if a.full else None  # (the roofline's bytes read)
    else:
        del first
        h_in = None
        out = DecodedBatch.allocate(nb, cap, dev, meta=meta)
    gathered = torch.zeros(world * 4, dtype=torch.int64, device=dev) if world > 1 else None
    if world > 1 and a.dist_backend == "gloo":  # (gloo gathers host tensors)
        gathered = gathered.cpu()

    def concat():
        # offset concat: all-gather per-rank totals (n_kv, key, val, restarts), rebase on device
        tot = out.totals[:32].view(torch.int64)
        if a.dist_backend == "gloo":
            concat_step(dist, gathered, tot.cpu(), lambda g: offset_concat(out, g.to(dev), rank, stream))
        else:
            concat_step(dist, gathered, tot, lambda g: offset_concat(out, g, rank, stream))

    def launch():
        if plan is not None:
            plan.launch(stream)
        else:
            decode_into(batch, out, stream)

    def step():
        launch()
        if world > 1:
            concat()

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize(dev)
    if a.warmup:
        t = out.read_totals()
        assert t.n_kv == n_kv and t.status_mask == 0, (t.n_kv, n_kv, t.status_mask)

    # kernel-only timing with HIP events on the launch stream
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t_start = time.perf_counter()
    for i in range(a.steps):
        ev[i][0].record(stream)
        launch()
        ev[i][1].record(stream)
        if world > 1:
            concat()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t_start
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    total_input = int(sum(rank_bytes))
    value = total_input * a.steps / elapsed / 2**30
    res = {
        "metric": METRIC, "value": round(value, 2), "unit": "GiB/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": wl,
                   "blocks_per_gpu": nb, "input_bytes_per_gpu": input_bytes, "kvs_per_gpu": n_kv,
                   "global_batch_blocks": int(shard_range[2]), "shard_blocks": [int(shard_range[0]), int(shard_range[1])],
                   "input_bytes_per_rank": [int(x) for x in rank_bytes],
                   "parallelism": f"shard{world}" + (f"+{'rccl' if a.dist_backend == 'nccl' else 'gloo'}_offset_concat"
                                                      if world > 1 else "")},
    }

    if a.dump_outputs and rank == 0:
        dump_outputs(out, a.dump_outputs)

    if a.full:
        kern_ms = float(np.mean([s.elapsed_time(e) for s, e in ev]))
        if world > 1:
            km = torch.tensor([kern_ms], dtype=torch.float64, device=dev)
            dist.all_reduce(km, op=dist.ReduceOp.MAX)
            kern_ms = float(km.item())
        hres = out.to_host()  # the whole output, checked against the generator's count
        assert hres["n_kv"] == n_kv and hres["status_mask"] == 0
        res["roofline"] = roofline(a, kernel, nb, input_bytes, kern_ms, hres, h_in)

    if a.full and rank == 0 and not a.no_cpu_baseline and plan is None:
        res["cpu_baseline"] = cpu_baseline(a, buf, off, lens, fmt, block_fmt, flags & 0xFF)

    if a.full and not a.no_e2e and rank == 0 and plan is None:
        del out  # (HBM for the pipeline's slots)
        torch.cuda.empty_cache()
        res["e2e_pcie"] = e2e_rate(buf, off, lens, flags & ~(N.PBL_BATCH_VARLEN | N.PBL_COL_TIERING), dev, cap, fmt,
                                   block_fmt, hres,
                                   chunk=a.e2e_chunk)

    res["gen_seconds"] = round(gen_s, 2)
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


SRC = {0: "oracle/rowblk_oracle.c (rowblk.Iter)",
       2: "oracle/colblk_oracle.c (colblk.DataBlockIter, crdb1)",
       1: "oracle/colblk_oracle.c (colblk.DataBlockIter, DefaultKeySchema)"}


def cpu_baseline(a, buf, off, lens, fmt, block_fmt, flags) -> dict:
    """The oracle's C restatement timed on this host (reported, not the
    target).  Streaming: every pass reads the WHOLE batch once (2 GiB at
    configs 2/3, far past the host's L3), passes repeated to about
    --cpu-baseline-seconds.  The cache-resident rate (the first 4096 blocks
    repeated) is kept as a labelled extra."""
    import oracle
    oracle.build()
    th, visible = cpu_threads(a)
    nb = len(off)
    parts = []
    for f in ([fmt] if block_fmt is None else sorted(set(int(x) for x in np.unique(block_fmt)))):
        ids = np.arange(nb) if block_fmt is None else np.nonzero(block_fmt == f)[0]
        parts.append((f, np.ascontiguousarray(off[ids]), np.ascontiguousarray(lens[ids])))
    budget = a.cpu_baseline_seconds / len(parts)
    it_bytes = it_sec = m_bytes = m_sec = c_bytes = c_sec = 0.0
    reps_used = []
    for f, po, pl in parts:
        pbytes = float(pl.astype(np.int64).sum())
        t1 = oracle.bench(buf, po, pl, f, flags, th, 0, 1)
        reps = max(1, int(budget * 0.6 / max(t1, 1e-3)))
        it_sec += oracle.bench(buf, po, pl, f, flags, th, 0, reps)
        it_bytes += pbytes * reps
        reps_used.append(reps)
        mr = max(1, reps // 4)
        m_sec += oracle.bench(buf, po, pl, f, flags, th, 1, mr)
        m_bytes += pbytes * mr
        # cache-resident extra: the first 4096 blocks of this format, repeated
        co, cl = po[:4096], pl[:4096]
        cb = float(cl.astype(np.int64).sum())
        tc = oracle.bench(buf, co, cl, f, flags, th, 0, 1)
        cr = max(1, int(budget * 0.2 / max(tc, 1e-4)))
        c_sec += oracle.bench(buf, co, cl, f, flags, th, 0, cr)
        c_bytes += cb * cr
    share = os.environ.get("OMP_NUM_THREADS")
    return {
        "value": round(it_bytes / it_sec / 2**30, 2), "unit": "GiB/s", "cores": th, "kind": "port",
        "sample": (f"whole batch streamed ({it_bytes / max(1, sum(reps_used)) / 2**30:.2f} GiB per pass, "
                   f"{reps_used} passes, {it_bytes / 2**30:.1f} GiB in all, past the host L3), iterate-only (Go "
                   f"iterator semantics: key materialized into a reused buffer, value zero-copy, checksum), "
                   f"C restatement {' + '.join(SRC[f] for f, _, _ in parts)}, one block per task on {th} threads"),
        "host_cpus_visible": visible,
        "threads_note": (f"capped at the box's CPU share OMP_NUM_THREADS={share}" if share and th < visible
                         else "every CPU this process may run on"),
        "materialize_value": round(m_bytes / m_sec / 2**30, 2),
        "cache_resident_value": round(c_bytes / c_sec / 2**30, 2),
        "cache_resident_sample": "first 4096 blocks of each format (128 MiB) repeated: an L3-resident upper bound",
        "host_cpu": _cpu_model(), "seconds": round(it_sec + m_sec + c_sec, 2),
    }


def config1(a) -> None:
    """BASELINE config 1: one 32 KiB row block (restart interval 16, 16 B keys /
    100 B values) iterated on the CPU the way BenchmarkBlockIterNext does
    (sstable/rowblk/rowblk_bench_test.go:81-244): the oracle's iterate-only
    loop, one thread, the block L1/L2-resident; plus the same block through the
    device decode (one launch, HIP events) as the plumbing comparison."""
    import oracle
    from pebble_amd import _native as N
    from pebble_amd.rowblk import gen_row_blocks
    oracle.build()
    buf, off, lens, n_kv = gen_row_blocks(a.seed, 1, 32768, a.restart_interval, a.key_len, a.val_len, False)
    reps = 20000
    oracle.bench(buf, off, lens, 0, 0, 1, 0, 1000)
    sec = oracle.bench(buf, off, lens, 0, 0, 1, 0, reps)
    ns_block = sec / reps * 1e9
    res = {"metric": METRIC, "value": round(float(lens[0]) / (sec / reps) / 2**30, 3), "unit": "GiB/s",
           "n_gpus": 0, "steps": reps, "warmup": 1000, "ms_per_step": round(sec / reps * 1e3, 6),
           "higher_is_better": True, "scaling": "none", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
           "config": {"workload": f"config1: one {int(lens[0])} B row block, restart interval {a.restart_interval}, "
                                  f"{a.key_len} B keys / {a.val_len} B values, {n_kv} KVs; CPU iterate-only "
                                  f"(oracle/rowblk_oracle.c, one thread)", "parallelism": "none"},
           "ns_per_block": round(ns_block, 1), "ns_per_kv": round(ns_block / n_kv, 2)}
    try:
        if torch.cuda.is_available():
            from pebble_amd.batch import BlockBatch, decode, decode_into
            dev = torch.device("cuda", 0)
            b = BlockBatch.from_host(buf, off, lens, dev)
            out = decode(b)
            st = torch.cuda.current_stream(dev)
            for _ in range(20):
                decode_into(b, out, st)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(200):
                decode_into(b, out, st)
            e1.record(st)
            torch.cuda.synchronize(dev)
            res["gpu_single_block_us"] = round(e0.elapsed_time(e1) / 200 * 1e3, 2)
            res["gpu_note"] = "one block per launch: launch-latency bound plumbing, not a throughput figure"
    except Exception as e:  # the CPU figure is the config's measurement
        res["gpu_note"] = f"gpu leg skipped: {e}"
    print(json.dumps(res), flush=True)


def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def e2e_rate(buf, off, lens, flags, dev, cap, fmt=0, block_fmt=None, hres=None, passes=2, chunk=2048):
    """PCIe-inclusive rate (pebble_amd/pipeline.py): pinned host blocks -> H2D
    -> decode -> exact-size D2H of trailers, flags, key/value offsets and key /
    value bytes, full duplex on three streams with three chunk slots.  Value =
    raw block bytes per second of the whole pass.  The copy engines' own rates
    (1 GiB H2D, D2H, and both at once) are reported beside it."""
    from pebble_amd.pipeline import stream_batch
    nb = len(off)
    hi = int((off.astype(np.uint64) + lens.astype(np.uint64)).max())
    host_in = torch.from_numpy(buf[:hi]).pin_memory()
    in_bytes = int(lens.astype(np.int64).sum())
    outs, _, pipe = stream_batch(host_in, off, lens, fmt, flags, cap, dev, chunk_blocks=chunk,
                                 block_format=block_fmt)  # warm
    if hres is not None:  # chunk 0's host arrays equal the device-resident decode
        c0 = outs.chunks[0]
        assert np.array_equal(outs.view(0, "val_bytes", np.uint8), hres["val_bytes"][:c0.val_bytes])
        assert np.array_equal(outs.view(0, "key_bytes", np.uint8), hres["key_bytes"][:c0.key_bytes])
        assert np.array_equal(outs.view(0, "trailer", np.uint64), hres["trailer"][:c0.n_kv])
    secs = []
    for _ in range(passes):
        outs, dt, pipe = stream_batch(host_in, off, lens, fmt, flags, cap, dev, block_format=block_fmt, pipe=pipe,
                                      outputs=outs)
        secs.append(dt)
    d2h = sum(c.n_kv * 17 + 8 * c.n_blocks + c.key_bytes + c.val_bytes for c in outs.chunks)
    dt = min(secs)

    # copy-engine reference rates
    g = 1 << 30
    hsrc = host_in[:g] if host_in.numel() >= g else host_in
    n = hsrc.numel()
    dbuf = torch.empty(n, dtype=torch.uint8, device=dev)
    dsrc = torch.empty(n, dtype=torch.uint8, device=dev)
    hdst = torch.empty(n, dtype=torch.uint8).pin_memory()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t

    def both():
        with torch.cuda.stream(s1):
            dbuf.copy_(hsrc, non_blocking=True)
        with torch.cuda.stream(s2):
            hdst.copy_(dsrc, non_blocking=True)
    t_h2d = timed(lambda: dbuf.copy_(hsrc, non_blocking=True))
    t_d2h = timed(lambda: hdst.copy_(dsrc, non_blocking=True))
    t_both = timed(both)
    del dbuf, dsrc, hdst, pipe
    torch.cuda.empty_cache()
    return {"value": round(in_bytes / dt / 2**30, 2), "unit": "GiB/s", "passes_s": [round(x, 4) for x in secs],
            "h2d_bytes": in_bytes, "d2h_bytes": int(d2h),
            "link_GB_per_s_both_directions": round((in_bytes + d2h) / dt / 1e9, 1),
            "copy_engine_GB_per_s": {"h2d": round(n / t_h2d / 1e9, 1), "d2h": round(n / t_d2h / 1e9, 1),
                                     "h2d+d2h_concurrent": round(2 * n / t_both / 1e9, 1)},
            "note": (f"pinned host blocks -> H2D -> decode -> exact-size D2H (trailer, kv_flags, key_off, val_off, "
                     f"key and value bytes); {chunk}-block chunks, 3 slots, separate H2D / decode / D2H streams, the "
                     "host waits only on a chunk's totals after queueing the next two; best of "
                     f"{passes} warm passes; chunk 0 checked against the device-resident decode")}


if __name__ == "__main__":
    main()
