"""ns_cluster_grid / ns_cluster_place (csrc/exchange.h), the one map from a grid index to (cluster, member) that every
cluster kernel and its launcher share, reached through the two host queries of include/nspeech_hip.h.  Pure host code:
no device is needed."""
import ctypes

import pytest

from nspeech_amd import _lib

MEMBERS = (2, 4, 8, 16)
CLUSTERS = range(1, 41)


def _grid(clusters, members, placed):
    return _lib.lib().ns_cluster_grid_query(clusters, members, int(placed))


def _place(b, clusters, members, placed):
    c, m = ctypes.c_int(-1), ctypes.c_int(-1)
    active = _lib.lib().ns_cluster_place_query(b, clusters, members, int(placed), ctypes.byref(c), ctypes.byref(m))
    assert active in (0, 1), _lib.lib().ns_last_error()
    return bool(active), c.value, m.value


def test_exported():
    for f in ("ns_cluster_grid_query", "ns_cluster_place_query", "ns_cluster_probe"):
        assert f in _lib.FUNCS and hasattr(_lib.lib(), f), f
    c = ctypes.c_int()
    assert _lib.lib().ns_cluster_grid_query(4, 0, 1) == -1                                 # members < 1: an argument error
    assert _lib.lib().ns_cluster_place_query(0, 4, 4, 1, None, ctypes.byref(c)) == -1     # so is a null out


@pytest.mark.parametrize("members", MEMBERS)
def test_placed_map(members):
    for clusters in CLUSTERS:
        grid = _grid(clusters, members, True)
        assert grid == 8 * members * ((clusters + 7) // 8), (clusters, grid)
        if clusters % 8 == 0:
            assert grid == clusters * members, (clusters, grid)
        seen, residue = set(), {}
        for b in range(grid):
            active, c, m = _place(b, clusters, members, True)
            if not active:
                assert c >= clusters, (clusters, b, c)       # every other index is inactive: its cluster does not exist
                continue
            assert 0 <= c < clusters and 0 <= m < members, (clusters, b, c, m)
            assert (c, m) not in seen, (clusters, b, c, m)
            seen.add((c, m))
            assert residue.setdefault(c, b % 8) == b % 8, (clusters, b, c)      # one residue per cluster
        assert len(seen) == clusters * members, (clusters, len(seen))      # one-to-one onto clusters x members
        assert _place(0, clusters, members, True) == (True, 0, 0)


@pytest.mark.parametrize("members", MEMBERS)
def test_linear_map(members):
    for clusters in CLUSTERS:
        grid = _grid(clusters, members, False)
        assert grid == clusters * members, (clusters, grid)
        for b in range(grid):
            assert _place(b, clusters, members, False) == (True, b // members, b % members), (clusters, b)
        assert not _place(grid, clusters, members, False)[0]
