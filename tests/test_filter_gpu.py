"""pbl_filter_probe on the device against pbl_filter_probe_host: `may`, `hash`
and `flt_status` are equal exactly, on every filter shape and key of
tests/test_filter.py, at batch sizes around the wave (1, 63, 64, 65, 257), in
named and all-pairs mode with 1, 2 and 5 filters, keys given as a list and as
device tensors."""
import numpy as np
import pytest
import torch

import filterutil as FU
from pebble_amd import _native as N
from pebble_amd import filter as F
from pebble_amd.seek import pack_keys

pytestmark = pytest.mark.gpu

G = FU.load_golden()
CASES = FU.filter_cases()
BY_NAME = {c[0]: c for c in CASES}


def _device(r):
    torch.cuda.synchronize()
    return (r.may.cpu().numpy(), r.hash.cpu().numpy().view(np.uint32), r.status.cpu().numpy())


def _same(dev, host, ctx=""):
    for a, b, what in zip(dev, host, ("may", "hash", "status")):
        assert a.shape == b.shape and np.array_equal(a, b), (ctx, what)


def test_hash_vectors_and_every_tail_length():
    keys = [bytes.fromhex(v["key"]) for v in G["hash"]] + FU.edge_keys()
    d = _device(F.probe([BY_NAME["bpk10_lines3"][1]], keys, N.PBL_CMP_DEFAULT))
    _same(d, F.probe_host([BY_NAME["bpk10_lines3"][1]], keys, N.PBL_CMP_DEFAULT))
    assert d[1][:41].tolist() == [v["hash"] for v in G["hash"]]


def test_small_filter_answers():
    s = G["small"]
    names = sorted(s["answers"])
    d = _device(F.probe([bytes.fromhex(s["filter_hex"])], [k.encode() for k in names], N.PBL_CMP_DEFAULT))
    assert [bool(m) for m in d[0][0]] == [s["answers"][k] for k in names]


@pytest.mark.parametrize("name,flt,members", CASES, ids=[c[0] for c in CASES])
def test_every_filter_shape(name, flt, members):
    keys = FU.probe_keys(members)
    _same(_device(F.probe([flt], keys, N.PBL_CMP_DEFAULT)), F.probe_host([flt], keys, N.PBL_CMP_DEFAULT), name)


def _keys(n):
    m = BY_NAME["bpk10_lines35"][2] + BY_NAME["bpk5_lines3"][2] + BY_NAME["bpk20_lines1"][2]
    return [m[(i * 13) % len(m)] if i % 3 else b"nk%05d" % i for i in range(n)]


FILTERS = [BY_NAME[n][1] for n in ("bpk10_lines35", "bpk5_lines3", "lines_mismatch", "len5", "bpk20_lines1")]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nf", [1, 2, 5])
def test_partial_waves_both_modes(n, nf):
    flts, keys = FILTERS[:nf], _keys(n)
    _same(_device(F.probe(flts, keys, N.PBL_CMP_DEFAULT)), F.probe_host(flts, keys, N.PBL_CMP_DEFAULT), "all pairs")
    # named: ids that differ inside a wave, some of them past the filters
    which = [(i * 7) % (nf + 1) for i in range(n)]
    _same(_device(F.probe(flts, keys, N.PBL_CMP_DEFAULT, which=which)),
          F.probe_host(flts, keys, N.PBL_CMP_DEFAULT, which=which), "named, mixed")
    # named: one id for the whole batch (the wave-uniform path), a valid one and one past the filters
    for w in (nf - 1, nf):
        _same(_device(F.probe(flts, keys, N.PBL_CMP_DEFAULT, which=[w] * n)),
              F.probe_host(flts, keys, N.PBL_CMP_DEFAULT, which=[w] * n), f"named, all {w}")


def test_keys_and_filters_as_device_tensors():
    flts, keys = FILTERS, _keys(257)
    hb, ho = pack_keys(keys)
    kb = torch.from_numpy(hb).cuda()
    ko = torch.from_numpy(ho.view(np.int64)).cuda()
    dflts = [torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda() for f in flts]
    which = torch.tensor([(i * 3) % 5 for i in range(257)], dtype=torch.int32, device="cuda")
    host = F.probe_host(flts, keys, N.PBL_CMP_DEFAULT)
    _same(_device(F.probe(dflts, (kb, ko), N.PBL_CMP_DEFAULT)), host)
    _same(_device(F.probe([dflts[0], flts[1], dflts[2], flts[3], dflts[4]], (kb, ko), N.PBL_CMP_DEFAULT)), host)
    _same(_device(F.probe(dflts, (kb, ko), N.PBL_CMP_DEFAULT, which=which)),
          F.probe_host(flts, keys, N.PBL_CMP_DEFAULT, which=which.cpu().numpy()))


@pytest.mark.parametrize("comparer", [N.PBL_CMP_TESTKEYS, N.PBL_CMP_CRDB])
def test_split_prefixes(comparer):
    if comparer == N.PBL_CMP_TESTKEYS:
        keys = [b"a@5", b"a@9", b"b@5", b"a", b"", b"@3", b"abcdefghijklmnopqrstuvwxyz@12"]
    else:
        ver = lambda w: w.to_bytes(8, "big") + b"\x09"  # noqa: E731
        keys = [b"a\x00" + ver(5), b"a\x00" + ver(9), b"b\x00" + ver(5), b"a\x00", b"", b"\x09",
                b"abcdefghijklmnopqrstuvwxyz\x00" + ver(77)]
    f = F.build_host(keys[:1] + keys[-1:], comparer, 10)
    d = _device(F.probe([f], keys, comparer))
    _same(d, F.probe_host([f], keys, comparer))
    assert d[1][0] == d[1][1] and d[0][0][:3].tolist() == [1, 1, 0]


def test_empty_batches_launch_nothing():
    r = F.probe([FILTERS[0]], [], N.PBL_CMP_DEFAULT)
    assert r.may.numel() == 0 and r.hash.numel() == 0
