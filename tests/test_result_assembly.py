"""The workspace sizes of the batched scan, merge and visible view without a
GPU.  The three operators share the code that assembles a result
(pebble_amd/csrc/result_core.hip.h) but each keeps its own workspace layout;
the sizes below are those of the build before that code was shared, as
literals, so that a layout cannot move unnoticed."""
from pebble_amd import _native as N

WS = [  # ((blocks, KVs), scan with as many queries as blocks, merge, view)
    ((0, 0), 304, 128, 224),
    ((0, 255), 304, 4208, 10688),
    ((0, 256), 320, 4240, 10768),
    ((0, 257), 320, 4256, 10816),
    ((255, 0), 30896, 8304, 8400),
    ((255, 255), 30896, 12384, 18848),
    ((255, 256), 30928, 12416, 18928),
    ((255, 257), 30928, 12432, 18976),
    ((256, 0), 31024, 8320, 8416),
    ((256, 255), 31024, 12400, 18880),
    ((256, 256), 31040, 12432, 18960),
    ((256, 257), 31040, 12448, 19008),
    ((257, 0), 31168, 8384, 8480),
    ((257, 255), 31168, 12464, 18944),
    ((257, 256), 31200, 12496, 19024),
    ((257, 257), 31200, 12512, 19072),
    ((100000, 4294979641), 481776560, 68991319968, 176770824736),
]
SCAN_Q = [  # ((queries, blocks, KVs), scan)
    ((0, 7, 1000), 592),
    ((255, 1, 70000), 30416),
    ((256, 3, 0), 22928),
    ((257, 300, 65536), 39712),
    ((1000, 0, 0), 88400),
]


def test_workspace_sizes_are_what_they_were():
    L = N.lib()
    for (nb, n_kv), s, m, v in WS:
        assert int(L.pbl_scan_workspace_bytes(nb, nb, n_kv)) == s, ("scan", nb, n_kv)
        for n_runs in (1, 2, 16):  # nothing in the merge's workspace scales with the runs
            assert int(L.pbl_merge_workspace_bytes(n_runs, nb, n_kv)) == m, ("merge", n_runs, nb, n_kv)
        assert int(L.pbl_visible_workspace_bytes(nb, n_kv)) == v, ("visible", nb, n_kv)
    for (nq, nb, n_kv), s in SCAN_Q:
        assert int(L.pbl_scan_workspace_bytes(nq, nb, n_kv)) == s, ("scan", nq, nb, n_kv)
