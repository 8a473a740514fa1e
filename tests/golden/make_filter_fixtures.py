#!/usr/bin/env python3
"""Bloom filter fixtures, read from the reference AS DATA (test infrastructure;
run once where the reference checkout is at hand, outputs committed):

  sstable/testdata/h-table-bloom-no-compression-sst/000011.sst -> tests/golden/sst/h_bloom_no_compression.sst
  sstable/testdata/h-table-bloom-sst/000010.sst                -> tests/golden/sst/h_bloom_snappy.sst
  sstable/tablefilters/bloom/bloom_test.go                     -> tests/golden/filter.json
      TestHash's 41 (key, hash) pairs; TestSmallBloomFilter's bit picture (69
      bytes, "hello" and "world" at 10 bits per key) with its four answers

filter.json also records, per table, the filter block's handle (read from the
metaindex), its trailer (nLines, nProbes), and the number of false positives
among the 10 000 keys "m!" + LE32(i) of TestBloomFilterFalsePositiveRate
(sstable/table_test.go:324-369), counted with tests/filterutil.py and checked
against the range that test accepts (0.2 % to 5 %).

usage: make_filter_fixtures.py <path of the reference checkout>
"""
import json
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import filterutil as FU  # noqa: E402
import oracle  # noqa: E402

TABLES = {"h_bloom_no_compression": "sstable/testdata/h-table-bloom-no-compression-sst/000011.sst",
          "h_bloom_snappy": "sstable/testdata/h-table-bloom-sst/000010.sst"}
FILTER_NAME = b"fullfilter.rocksdb.BuiltinBloomFilter"


def hash_vectors(src: str):
    body = src[src.index("func TestHash"):]
    out = [{"key": re.sub(r"\\x", "", k), "hash": int(h)}
           for k, h in re.findall(r'\{"((?:\\x[0-9a-f]{2})*)", (\d+)\}', body)]
    assert len(out) == 41
    return out


def small_filter(src: str):
    body = src[src.index("func TestSmallBloomFilter"):]
    pic = body[body.index("want := `") + 9:]
    pic = pic[:pic.index("`")]
    bits = re.findall(r"[.1]{8}", pic)
    data = bytes(int(b.replace(".", "0"), 2) for b in bits)  # filterStr prints bit 7 first
    assert len(data) == 69
    ans = {k: v == "true" for k, v in re.findall(r'"(\w+)":\s+(true|false),', body[:body.index("for k, want")])}
    assert ans == {"hello": True, "world": True, "x": False, "foo": False}
    return {"keys": ["hello", "world"], "bits_per_key": 10, "filter_hex": data.hex(), "answers": ans}


def table_entry(data: bytes):
    f = oracle.parse_footer(data[-61:], len(data))
    st, rows = oracle.rowblk_decode_block(oracle.table_block(data, f["metaindex"], f["checksum_type"]), 0x4)[:2]
    assert st == 0
    meta = {r[0]: oracle.decode_handle(r[2], 0)[0] for r in rows}
    h = meta[FILTER_NAME]
    flt = oracle.table_block(data, h, f["checksum_type"])
    n_lines, n_probes, status = FU.parse(flt)
    assert status == FU.OK
    fp = sum(FU.may_bits(flt, FU.bloom_hash(b"m!" + i.to_bytes(4, "little"))) & 1 for i in range(10000))
    assert 0.002 * 10000 <= fp <= 0.05 * 10000
    return {"filter_handle": list(h), "n_lines": n_lines, "n_probes": n_probes, "false_positives_m": fp}


def main(ref: str):
    src = open(os.path.join(ref, "sstable/tablefilters/bloom/bloom_test.go")).read()
    out = {"hash": hash_vectors(src), "small": small_filter(src), "tables": {}}
    for name, rel in TABLES.items():
        dst = os.path.join(HERE, "sst", name + ".sst")
        shutil.copyfile(os.path.join(ref, rel), dst)
        os.chmod(dst, 0o644)
        out["tables"][name] = table_entry(open(dst, "rb").read())
    with open(os.path.join(HERE, "filter.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
