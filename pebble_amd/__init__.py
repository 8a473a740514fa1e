"""pebble_amd — MI355X-native decoder for Pebble SSTable data blocks.

The hot path (raw data blocks in HBM -> flat key / value / offset arrays) runs in
hand-written gfx950 HIP kernels inside libpebble_amd.so, reached through the
C-ABI declared in include/pebble_amd.h.  This package is the host layer:

  pebble_amd.batch   BlockBatch / decode() / DecodedBatch (device buffers, streams)
  pebble_amd.rowblk  Writer, NewIter/Iter mirroring sstable/rowblk
  pebble_amd.shard   multi-GPU sharding + RCCL offset concat
  pebble_amd.seek    batched SeekGE / SeekLT over a DecodedBatch, on the device
  pebble_amd.scan    batched bounded scans over a DecodedBatch, on the device
  pebble_amd.merge   batched k-way merge of sorted DecodedBatches, on the device
  pebble_amd.visible the snapshot-visible view of a sorted DecodedBatch, and read()
  pebble_amd.compact the compaction view of a sorted DecodedBatch (what compact.Iter keeps), and compact_tables()
  pebble_amd.rangedel range deletions in that path: the flattened set and the per-KV cover
  pebble_amd.rangekey range keys in that path: the coalesced set at a snapshot (host), the per-KV mask (device)
  pebble_amd.keyspan columnar keyspan blocks into runs, on the device; Writer for tests and tools
"""
from . import _native  # noqa: F401

__all__ = ["batch", "rowblk", "build"]
