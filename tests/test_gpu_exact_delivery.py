"""GPU tests of spe_table_opts.exact_delivery: the default (shared / derived)
rows with every offset entry whose latency lies at an ns boundary re-folded in path order,
so that ceil(latency * 1e6) -- Shadow's packet delay, shd-worker.c:244 -- equals the
exact_sources = 1 build's for every entry, and flagged entries equal it bit for bit.

Shapes and weightings: tests/exact_delivery_cases.py.  On the grid weighting every path sum
is at an ns boundary, so every offset entry is flagged and the delivery table's latencies
are the exact build's bits; the default build moves ~20 % of the delays there (the premise
of test 1).  The reference is the exact_sources = 1 build of the same table (bit-exact
against the oracle: tests/test_gpu_parity.py, tests/test_gpu_derived.py).

fallback_blocks of the DEFAULT build with the grid weighting (one edge off the grid), for
the seeds in exact_delivery_cases.SEEDS, (groups 0, groups 6), measured on an MI355X:
  a (31, 131): (0, 0) of 47 blocks;  b (43, 143): (2, 0) of 54;  c (35, 135): (0, 0) of 47.
"""
import numpy as np
import pytest

import exact_delivery_cases as ec

pytestmark = [pytest.mark.gpu, pytest.mark.engine_fixed, pytest.mark.shared_trees]

SHAPES = ("a", "b", "c")


@pytest.fixture(scope="module")
def spe():
    from shadow_amd import spe as m
    assert m.device_count() > 0, "no GPU visible"
    return m


class Built:
    """Graph + default / exact / delivery tables of one case (built once per module)."""

    def __init__(self, spe, top, A, groups, **delivery_kw):
        self.g = spe.Graph(top)
        self.A = self.g.order_sources(A)
        kw = dict(engine=spe.SPE_ENGINE_BATCH, groups=groups)
        self.default = spe.PathTable(self.g, self.A, **kw)
        self.sd = self.default.build()
        self.exact = spe.PathTable(self.g, self.A, exact_sources=True, **kw)
        self.se = self.exact.build()
        self.delivery = spe.PathTable(self.g, self.A, exact_delivery=True, **delivery_kw, **kw)
        self.sx = self.delivery.build()


_cache = {}


def grid_built(spe, name, groups):
    """Test 1's tables (grid, one edge off it, delivery_refold_max = 1.0), shared with tests 3 and 5."""
    key = (name, groups)
    if key not in _cache:
        top, A = ec.grid_case(name)
        _cache[key] = Built(spe, top, A, groups, delivery_refold_max=1.0)
    return _cache[key]


@pytest.mark.parametrize("groups", [0, 6])
@pytest.mark.parametrize("name", SHAPES)
def test_grid_every_offset_entry_refolded(spe, name, groups):
    b = grid_built(spe, name, groups)
    lay = b.default.layout()
    nblk = b.default.nblocks
    # the default build really keeps its shared / derived rows (no pass by falling back) ...
    assert b.sd["derived_sources"] > 0 or lay["shared_sources"] == 1, (b.sd, lay)
    assert b.sd["fallback_blocks"] <= nblk // 2, b.sd
    assert b.sd["relaxed_lanes"] < len(b.A)
    # ... and really moves packet delays on these inputs: what is being fixed
    de = b.default.compare(b.exact)
    assert de["route_mismatch"] == 0 and de["delivery_flips"] > 0, de
    xe = b.delivery.compare(b.exact)
    print(name, groups, "default/exact", de, "delivery/exact", xe, "stats", b.sx)
    assert xe["route_mismatch"] == 0 and xe["delivery_flips"] == 0 and xe["latency_differs"] == 0, xe
    assert b.sx["delivery_changed"] == de["latency_differs"], (b.sx, de)
    xd = b.delivery.compare(b.default)
    assert xd["route_mismatch"] == 0 and xd["reliability_differs"] == 0, xd
    dd, dx = b.default.digest(), b.delivery.digest()
    np.testing.assert_array_equal(dx[:, 1:], dd[:, 1:])   # reliability, next hop, hops: the default's
    assert b.sx["delivery_fallback"] == 0
    assert b.sx["fallback_blocks"] == b.sd["fallback_blocks"] and b.sx["relaxed_lanes"] == b.sd["relaxed_lanes"]
    assert b.sx["delivery_flagged"] >= b.sx["delivery_changed"] > 0 and b.sx["delivery_seconds"] > 0


@pytest.mark.parametrize("name", SHAPES)
def test_all_on_grid_is_predicted_at_create(spe, name):
    top, A = ec.grid_case(name, off_grid_edge=False)
    g = spe.Graph(top)
    A = g.order_sources(A)
    t = spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True)
    st = t.build()
    assert st["delivery_fallback"] == 1 and st["relaxed_lanes"] == len(A) and st["derived_sources"] == 0, st
    assert st["delivery_flagged"] == 0 and st["delivery_changed"] == 0 and t.layout()["shared_sources"] == 0
    te = spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, exact_sources=True)
    te.build()
    np.testing.assert_array_equal(t.digest(), te.digest())


@pytest.mark.parametrize("name", SHAPES)
def test_blocks_over_the_cap_are_rebuilt(spe, name):
    b = grid_built(spe, name, 0)
    t = spe.PathTable(b.g, b.A, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True, delivery_refold_max=0.01)
    st = t.build()
    assert st["delivery_fallback"] == 2, st
    de, dd, dx = b.exact.digest(), b.default.digest(), t.digest()
    # every block that had offset rows: on the grid each of its offset entries is flagged, and one
    # offset source's A - 1 entries exceed the cap of 0.64 A.  Shape c's sources are all stubs
    # (every block); elsewhere at least the blocks whose default rows differ from the exact ones.
    had_offset = int((dd[:, 0] != de[:, 0]).sum())
    assert st["fallback_blocks"] >= had_offset > 0, (st, had_offset)
    if name == "c":
        assert st["fallback_blocks"] == t.nblocks
    np.testing.assert_array_equal(dx[:, 0], de[:, 0])      # latency digests of every block
    np.testing.assert_array_equal(dx[:, 2:], de[:, 2:])
    assert st["delivery_flagged"] >= b.sx["delivery_changed"], (st, b.sx)   # counted beyond the caps
    assert st["delivery_flagged"] == b.sx["delivery_flagged"]


@pytest.mark.parametrize("name", SHAPES)
def test_real_weights_keep_the_fast_path(spe, name):
    top, A = ec.shape(name)
    b = Built(spe, top, A, 0)
    xe = b.delivery.compare(b.exact)
    de = b.default.compare(b.exact)
    xd = b.delivery.compare(b.default)
    print(name, "default/exact", de, "delivery/exact", xe, "stats", b.sx)
    assert xe["route_mismatch"] == 0 and xe["delivery_flips"] == 0, xe
    assert b.sx["delivery_fallback"] == 0
    assert b.sx["delivery_flagged"] <= 1e-4 * xe["pairs"], (b.sx, xe["pairs"])
    assert xd["latency_differs"] <= b.sx["delivery_flagged"], (xd, b.sx)   # unflagged: the default's bits
    assert xd["reliability_differs"] == 0 and xd["route_mismatch"] == 0
    assert b.sx["relaxed_lanes"] == b.sd["relaxed_lanes"] < len(b.A)
    assert b.sx["fallback_blocks"] == b.sd["fallback_blocks"]


def test_block_ranges_and_caller_buffers(spe):
    import torch
    b = grid_built(spe, "a", 0)
    want = b.delivery.digest(1, 4)
    kw = dict(engine=spe.SPE_ENGINE_BATCH, exact_delivery=True, delivery_refold_max=1.0)
    t = spe.PathTable(b.g, b.A, **kw)
    st = t.build_blocks(1, 4)
    assert st["delivery_fallback"] == 0 and st["delivery_flagged"] > 0, st
    got = t.digest(1, 4)
    n = 3 * len(b.A) * 64
    bufs = [torch.zeros((n, 2), dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
            torch.zeros(n, dtype=torch.int16, device="cuda")]
    t2 = spe.PathTable(b.g, b.A, **kw)
    st2 = t2.build_blocks_into(1, 4, *[x.data_ptr() for x in bufs])
    assert st2["delivery_fallback"] == 0 and st2["delivery_flagged"] == st["delivery_flagged"], (st, st2)
    torch.cuda.synchronize()
    view = spe.PathTable(b.g, b.A, ext=[x.data_ptr() for x in bufs], ext_filled=True, blocks=(1, 4))
    into = view.digest()
    print("whole", want.tolist(), "blocks", got.tolist(), "into", into.tolist())
    np.testing.assert_array_equal(into, got)
    # Latency (on the grid every offset entry is re-folded to the exact bits), next hop and hops:
    # the whole delivery table's blocks 1-3.  Reliability is "what the default build writes", and
    # the default build of a block range does not write the whole build's bits: a source derived
    # in the whole build (a_leg * r_u(t)) relaxes on its own lane where the range lacks its
    # neighbours' roots (the path-order product), measured here: all three reliability digests
    # differ, on the parent commit's default build as well.  So that field is held, digest for
    # digest, to the default build of the same block range.
    for f in (0, 2, 3):
        np.testing.assert_array_equal(got[:, f], want[:, f])
    td = spe.PathTable(b.g, b.A, engine=spe.SPE_ENGINE_BATCH)
    td.build_blocks(1, 4)
    np.testing.assert_array_equal(got[:, 1], td.digest(1, 4)[:, 1])
    np.testing.assert_array_equal(want[:, 1], b.default.digest(1, 4)[:, 1])


def test_refusals_and_no_ops(spe):
    C = __import__("ctypes")
    top, A = ec.grid_case("a")
    g = spe.Graph(top)
    A = g.order_sources(A)

    def refused(option, **kw):
        with pytest.raises(spe.SpeError) as e:
            spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True, **kw)
        assert "(-4)" in str(e.value) and "exact_delivery" in str(e.value) and option in str(e.value), str(e.value)
        assert option.encode() in spe.lib().spe_last_error()

    refused("owner_rank", owner_order=np.arange(len(A)))
    g.set_edge_aux(np.ones(top.m))
    refused("want_aux", want_aux=True)
    refused("n_devices", devices=[0, 0])
    with pytest.raises(spe.SpeError):
        spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True, delivery_refold_max=1.5)

    def none(st):
        return (st["delivery_flagged"], st["delivery_changed"], st["delivery_fallback"], st["delivery_seconds"]) == (0, 0, 0, 0.0)

    # accepted and without effect: exact sources, the LDS and FW engines, DIRECT tables, exact sums
    t = spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True, exact_sources=True)
    assert none(t.build())
    for eng in (spe.SPE_ENGINE_LDS, spe.SPE_ENGINE_FW):
        t = spe.PathTable(g, A[:300], engine=eng, exact_delivery=True)
        assert none(t.build()), eng
    from shadow_amd import graphs
    n = 40
    iu = np.triu_indices(n)   # every pair and every self-loop: _topology_isComplete
    tc = graphs.Topology(n=n, esrc=iu[0].astype(np.int32), edst=iu[1].astype(np.int32),
                         elat=np.random.default_rng(2).uniform(1, 9, iu[0].shape[0]), eloss=np.zeros(iu[0].shape[0]),
                         vloss=np.zeros(n), directed=False, prefer_direct=False)
    gc = spe.Graph(tc)
    assert gc.info()["complete"] == 1
    t = spe.PathTable(gc, np.arange(n, dtype=np.int32), exact_delivery=True)
    assert none(t.build())
    ti, Ai = ec.shape("a")
    ti.elat = np.random.default_rng(5).integers(1, 30, ti.elat.shape[0]).astype(np.float64)
    gi = spe.Graph(ti)
    assert gi.info()["sums_exact"] == 1
    t = spe.PathTable(gi, Ai, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True)
    assert none(t.build()) and t.layout()["shared_sources"] == 1

    # the cache key: changes with exact_delivery, unchanged without it
    k0 = spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH).key()
    k1 = spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True).key()
    k2 = spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, exact_delivery=True, delivery_refold_max=0.5).key()
    assert k0 != k1 and k1 == k2
    assert k0 == spe.PathTable(g, A, engine=spe.SPE_ENGINE_BATCH, delivery_refold_max=0.5).key()
    assert C.sizeof(spe.TableOpts) == spe.TableOpts().struct_size
