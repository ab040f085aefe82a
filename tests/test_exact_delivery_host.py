"""CPU tests of spe_table_opts.exact_delivery's host parts: the boundary predicate
spe_delivery_near_boundary against numpy (soundness: every pair of folds of one path whose
ceil(L * 1e6) differ is flagged; selectivity on real-valued weights), and the ABI guard of
the two structs the option grew.

The model: a path of h edges is summed in path order from 0.0, (((0 + w_1) + w_2) + ...), as a
source's own relaxation lane does, and in offset order, leg + (((0 + w_k+1) + ...) + w_h) with
a one-edge (k = 1) or two-edge (k = 2, leg = (0 + w_1) + w_2) leg, as a shared / derived row
does: the root lane's distance summed from 0, the leg added in front.
"""
import ctypes

import numpy as np
import pytest

N = 2_000_000
CHUNK = 250_000   # rows folded at a time (80 MB of weights)
HMAX = 40


def near_np(lat, hops):
    """The predicate of include/spe.h, restated: x = L * 1e6, m = 4 (hops + 2) 2^-53 x,
    |x - rint(x)| <= m."""
    x = lat * 1e6
    m = ((4.0 * (hops + 2.0)) * 2.0 ** -53) * x
    return np.abs(x - np.rint(x)) <= m


def folds(w, hops):
    """Row i: a path of hops[i] edges w[i, :hops[i]].  Path-order sum and the offset sums
    with a one- and a two-edge leg."""
    n, hm = w.shape
    live = np.arange(hm)[None, :] < hops[:, None]
    w = np.where(live, w, 0.0)
    path = np.zeros(n)
    off1 = np.zeros(n)   # edges 2..h from 0
    off2 = np.zeros(n)   # edges 3..h from 0
    for k in range(hm):
        path = path + w[:, k]
        if k >= 1:
            off1 = off1 + w[:, k]
        if k >= 2:
            off2 = off2 + w[:, k]
    leg1 = 0.0 + w[:, 0]
    leg2 = (0.0 + w[:, 0]) + w[:, 1]
    return path, leg1 + off1, leg2 + off2


def weights(kind, rng, n):
    real = rng.uniform(1.0, 60.0, (n, HMAX))
    grid = rng.integers(100_000, 6_000_000, (n, HMAX)) * 1e-5
    if kind == "real":
        return real
    if kind == "grid":
        return grid
    return np.where(rng.random((n, HMAX)) < 0.5, real, grid)


@pytest.fixture(scope="module")
def lib():
    from shadow_amd import spe
    return spe.lib()


def c_near(lib, lat, hops):
    return np.array([lib.spe_delivery_near_boundary(float(a), int(h)) for a, h in zip(lat, hops)], bool)


@pytest.mark.parametrize("kind", ["real", "grid", "mixed"])
def test_predicate_flags_every_delivery_flip(lib, kind):
    rng = np.random.default_rng({"real": 1, "grid": 2, "mixed": 3}[kind])
    hops = rng.integers(2, HMAX + 1, N)
    parts = [folds(weights(kind, rng, CHUNK), hops[i:i + CHUNK]) for i in range(0, N, CHUNK)]
    path, off1, off2 = (np.concatenate([p[k] for p in parts]) for k in range(3))
    ns = lambda x: np.ceil(x * 1e6)
    flagged = 0
    for off in (off1, off2):
        flip = ns(off) != ns(path)
        # the entry a row kernel tests is the offset fold; the bound is symmetric, so the
        # path-order fold of a flipping pair satisfies it too
        assert near_np(off[flip], hops[flip]).all() and near_np(path[flip], hops[flip]).all(), kind
        idx = np.flatnonzero(flip)[:20000]
        assert c_near(lib, off[idx], hops[idx]).all(), kind            # ... by the library's own predicate
        flagged += int(near_np(off, hops).sum())
        print(kind, "flips", int(flip.sum()), "flagged share", near_np(off, hops).mean())
    if kind == "real":
        assert flagged / (2 * N) <= 1e-4
    if kind == "grid":
        assert flagged == 2 * N   # every sum of grid weights is at an ns boundary
    # the C predicate is the numpy restatement (a sample, and every flagged real-valued entry)
    idx = np.concatenate([rng.integers(0, N, 20000), np.flatnonzero(near_np(off1, hops))[:20000]])
    np.testing.assert_array_equal(c_near(lib, off1[idx], hops[idx]), near_np(off1[idx], hops[idx]))


def test_predicate_edges(lib):
    f = lib.spe_delivery_near_boundary
    assert f(12.345678, 3) == 1 and f(12.3456785, 3) == 0     # on / between ns boundaries
    assert f(1e-5, 1) == 1 and f(1.00000033, 1) == 0
    x = np.nextafter(12.345678, 13.0)
    assert f(float(x), 0) == 1                                 # one ulp off a boundary
    assert f(5000.00000033, 1) == 0


def test_stale_struct_size_of_the_grown_structs_is_refused_without_gpu():
    """A caller built against the spe.h before exact_delivery (structs 16 and 32 bytes
    shorter) is refused before anything else of it is read."""
    from shadow_amd import spe
    L = spe.lib()
    assert dict(spe.TableOpts._fields_).keys() >= {"exact_delivery", "delivery_refold_max"}
    assert dict(spe.BuildStats._fields_).keys() >= {"delivery_flagged", "delivery_changed", "delivery_fallback",
                                                    "delivery_seconds"}
    o = spe.TableOpts()
    o.struct_size = spe.TableOpts.exact_delivery.offset        # the previous sizeof(spe_table_opts)
    h = ctypes.c_void_p()
    att = np.zeros(1, np.int32)
    assert L.spe_table_create(None, att.ctypes.data, 1, ctypes.byref(o), ctypes.byref(h)) == -1
    assert b"struct_size" in L.spe_last_error() and b"spe_table_opts" in L.spe_last_error()
    o.struct_size = ctypes.sizeof(spe.TableOpts)               # the right size gets past the guard
    assert L.spe_table_create(None, att.ctypes.data, 1, ctypes.byref(o), ctypes.byref(h)) == -1
    assert b"struct_size" not in L.spe_last_error()
    s = spe.BuildStats()
    s.struct_size = spe.BuildStats.delivery_flagged.offset     # the previous sizeof(spe_build_stats)
    assert L.spe_table_build_stats(None, ctypes.byref(s)) == -1
    assert b"struct_size" in L.spe_last_error() and b"spe_build_stats" in L.spe_last_error()
    s.struct_size = ctypes.sizeof(spe.BuildStats)
    assert L.spe_table_build_stats(None, ctypes.byref(s)) == -1
    assert b"struct_size" not in L.spe_last_error()
