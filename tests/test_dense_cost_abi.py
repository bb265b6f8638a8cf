"""azd_debug_probe_dense_cost without a GPU: the symbol, and every argument check -- each made before a device is looked for, each
naming the graph it failed on (the kernel indexes LDS by the bits of adj and by the slots)."""
import numpy as np
import pytest

import dense_cost_cases as D


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


def probe(lib, graphs, n, toggles, count=None, n_toggles=None):
    from azdopt_amd import _lib
    adj = np.ascontiguousarray(graphs, dtype=np.uint64)
    tog = np.ascontiguousarray(toggles, dtype=np.uint16)
    count = len(graphs) if count is None else count
    k = (tog.shape[1] if tog.ndim == 2 else 0) if n_toggles is None else n_toggles
    rows = max(count, 1) * (max(k, 0) + 1)
    lam, mu, hooks, mate = np.zeros(rows), np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros((rows, 64), np.uint8)
    st = lib.azd_debug_probe_dense_cost(0, _lib.ptr(adj), n, count, _lib.ptr(tog) if tog.size else None, k, _lib.ptr(lam), _lib.ptr(mu), _lib.ptr(mate),
                                        _lib.ptr(hooks))
    return st, lib.azd_last_error().decode()


def test_symbol_is_exported_and_bound(lib):
    assert len(lib.azd_debug_probe_dense_cost.argtypes) == 10


def test_a_valid_call_passes_every_check(lib):
    good = D.from_edges(8, D.cycle(8))
    st, why = probe(lib, [good, good], 8, [[0, 5, 27], [3, 4, 9]])
    assert st in (0, 2), why  # ran, or "no device"
    st, why = probe(lib, [D.from_edges(64, D.complete(64))], 64, [[2015]])
    assert st in (0, 2), why


def test_each_rejection_is_an_invalid_argument_that_names_the_graph(lib):
    good = D.from_edges(8, D.cycle(8))
    seq = [0, 5, 27]

    def bad_graph(change):
        g = list(good)
        change(g)
        return [good, g]

    def loop(g):
        g[3] |= 1 << 3

    def asymmetric(g):
        g[2] |= 1 << 6

    def beyond_n(g):
        g[1] |= 1 << 8

    for change, word in ((loop, "loop"), (asymmetric, "symmetric"), (beyond_n, "above n")):
        st, why = probe(lib, bad_graph(change), 8, [seq, seq])
        assert st == 1 and "azd_debug_probe_dense_cost" in why and "graph 1" in why and word in why, (word, why)
    st, why = probe(lib, [good, good], 8, [seq, [0, 28, 5]])  # E = 28
    assert st == 1 and "graph 1" in why and "E" in why, why
    st, why = probe(lib, [good, good, good], 8, [seq, seq, [7, 5, 7]])
    assert st == 1 and "graph 2" in why and "twice" in why, why
    for n in (3, 65, 0, -1):
        st, why = probe(lib, [good], n, [seq])
        assert st == 1 and "n:" in why, (n, why)
    for count in (0, -2):
        st, why = probe(lib, [good], 8, [seq], count=count)
        assert st == 1 and "count" in why, why
    for k in (-1, 65):
        st, why = probe(lib, [good], 8, [list(range(28))], n_toggles=k)
        assert st == 1 and "n_toggles" in why, why
    from azdopt_amd import _lib
    out = np.zeros(64, np.uint8)
    assert lib.azd_debug_probe_dense_cost(0, None, 8, 1, None, 0, _lib.ptr(out), _lib.ptr(out), _lib.ptr(out), _lib.ptr(out)) == 1
