"""The device-side table utilities against the numpy reference of their contracts
(tests/table_reports.py, itself checked by hand in test_table_reports.py):
spe_table_compare, spe_table_check, spe_lookup_batch(_host), spe_table_min_latency,
spe_table_download / spe_table_get_row_latrel.

Everything the suite claims about whole tables ("the default build equals the
exact build on every entry", "every entry sane") is one of these kernels
reporting zeros; here they are shown to report the right non-zero numbers.  The
tables live in caller-owned storage (spe_table_opts.ext_*, ext_filled = 1), so a
test writes any SB64 content it likes -- garbage in the padding lanes included
-- from torch and predicts every counter with numpy.
"""
import numpy as np
import pytest

import table_reports as tr
from shadow_amd import graphs
from shadow_amd.graphs import Topology

pytestmark = [pytest.mark.gpu, pytest.mark.engine_fixed]

GRID_CAP = 16384 * 256          # threads of one pass of k_table_compare / k_table_check / k_lookup
MIN_CAP = 4096 * 256            # ... of k_min_latency
UNROUTABLE = {"lat": -1.0, "rel": -1.0, "next": -1, "hops": 0}


@pytest.fixture(scope="module")
def spe():
    from shadow_amd import spe as m
    assert m.device_count() > 0, "no GPU visible"
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as m
    return m


# ---- tables in torch-owned storage ---------------------------------------------------------

def ring(n):
    """Any valid graph over n vertices, for tables whose content is synthetic."""
    v = np.arange(n, dtype=np.int32)
    return Topology(n=n, esrc=v, edst=((v + 1) % n).astype(np.int32), elat=np.full(n, 1.0), eloss=np.zeros(n),
                    vloss=np.zeros(n))


def empty_bufs(torch, elems):
    return [torch.empty((elems, 2), dtype=torch.float64, device="cuda"),   # {latency, reliability}
            torch.empty(elems, dtype=torch.int32, device="cuda"),
            torch.empty(elems, dtype=torch.int16, device="cuda")]          # uint16 bit pattern


def upload(torch, rows, A, b0, b1, pad=None):
    """Row-major owned rows -> the three SB64 device tensors; padding lanes from
    `pad` (dict of span-shaped arrays; default: the unroutable entry)."""
    pad = pad or {}
    lr = tr.pack_sb64(np.stack([rows["lat"], rows["rel"]], -1), A, b0, b1, pad.get("lr", -1.0))
    nx = tr.pack_sb64(np.asarray(rows["next"], np.int32), A, b0, b1, pad.get("next", -1))
    hp = tr.pack_sb64(tr.hops_to_i16(rows["hops"]), A, b0, b1, pad.get("hops", 0))
    bufs = [torch.from_numpy(x).cuda() for x in (lr, nx, hp)]
    torch.cuda.synchronize()
    return bufs


def clone(torch, bufs):
    out = [b.clone() for b in bufs]
    torch.cuda.synchronize()
    return out


def copy_rows(rows):
    return {k: np.array(rows[k]) for k in tr.FIELDS}


def push(torch, bufs, new, old, A, b0=0):
    """Write the entries of `new` that differ from `old` (row-major owned rows of
    blocks from b0 on) into the device tensors, each at its SB64 offset."""
    ch = (tr._bits(new["lat"]) != tr._bits(old["lat"])) | (tr._bits(new["rel"]) != tr._bits(old["rel"])) | \
         (new["next"] != old["next"]) | (new["hops"] != old["hops"])
    s, t = np.nonzero(ch)
    o = torch.from_numpy(tr.sb64_offset(A, b0, s + b0 * tr.WAVE, t)).cuda()
    bufs[0][o, 0] = torch.from_numpy(new["lat"][s, t]).cuda()
    bufs[0][o, 1] = torch.from_numpy(new["rel"][s, t]).cuda()
    bufs[1][o] = torch.from_numpy(np.asarray(new["next"][s, t], np.int32)).cuda()
    bufs[2][o] = torch.from_numpy(tr.hops_to_i16(new["hops"][s, t])).cuda()
    torch.cuda.synchronize()
    return len(s)


def adopt(spe, g, attached, bufs, blocks=None):
    t = spe.PathTable(g, attached, ext=[b.data_ptr() for b in bufs], ext_filled=True, blocks=blocks)
    t._bufs = bufs   # the storage outlives the table
    return t


def owned(t, blocks=None):
    b0, b1 = blocks or (0, t.nblocks)
    return tr.owned_rows(t.A, b0, b1)


def download(t, blocks=None):
    r0, r1 = owned(t, blocks)
    d = t.download(r0, r1)
    return {k: d[k] for k in tr.FIELDS}


def garbage_pad(A, b0, b1, seed):
    """Padding-lane content that would count if a kernel read it: positive
    latencies and NaNs, reliabilities in and out of range, random routes."""
    rng = np.random.default_rng(seed)
    e = (b1 - b0) * A * tr.WAVE
    lr = rng.uniform(1e-3, 40.0, (e, 2))
    lr[rng.random(e) < 0.25] = np.nan
    return {"lr": lr, "next": rng.integers(-5, 10**6, e).astype(np.int32),
            "hops": rng.integers(-32768, 32768, e).astype(np.int16)}


def fill_padding(torch, bufs, A, b0, b1, seed):
    pm = torch.from_numpy(tr.padding_mask(A, b0, b1)).cuda()
    assert int(pm.sum()) > 0
    gp = garbage_pad(A, b0, b1, seed)
    for b, k in zip(bufs, ("lr", "next", "hops")):
        b[pm] = torch.from_numpy(gp[k]).cuda()[pm]
    torch.cuda.synchronize()


# ---- the base table R ------------------------------------------------------------------------

class Base:
    pass


@pytest.fixture(scope="module")
def R(spe, torch):
    """gen_random_small(300, 900), every vertex attached: 5 blocks, the last with
    44 real and 20 padding lanes; built once into torch-owned buffers."""
    from oracle import Oracle
    r = Base()
    r.top = graphs.gen_random_small(300, 900, 61)
    r.A = 300
    r.att = np.arange(r.A, dtype=np.int32)
    r.g = spe.Graph(r.top)
    r.bufs = empty_bufs(torch, 5 * r.A * 64)
    t = spe.PathTable(r.g, r.att, ext=[b.data_ptr() for b in r.bufs], exact_sources=True)
    t.build()
    torch.cuda.synchronize()
    r.rows = download(t)
    ref = Oracle(r.top).rows(r.att, r.att)
    ok = ref["kind"] != 0
    assert ok.all() and (r.rows["lat"] > -1.0).all()      # connected: every entry routable
    for k in tr.FIELDS:
        assert (r.rows[k] == ref[k]).all(), k
    r.table = t
    return r


def perturbed(spe, torch, R, new, blocks=None):
    """A clone of R's tensors holding `new` (whole-table row-major rows), adopted."""
    bufs = clone(torch, R.bufs)
    push(torch, bufs, new, R.rows, R.A)
    if blocks:
        e0, e1 = blocks[0] * R.A * 64, blocks[1] * R.A * 64
        bufs = [b[e0:e1] for b in bufs]
    return adopt(spe, R.g, R.att, bufs, blocks)


# ---- spe_table_compare -----------------------------------------------------------------------

def assert_compare(ta, tb, tol=1e-12, blocks=None, rows=None):
    """The device report of compare(ta, tb) equals compare_report of the two
    downloads (or of `rows`, what was uploaded), every field; returns (report, first_bad)."""
    got = ta.compare(tb, tol)
    da, db = rows or (download(ta, blocks), download(tb, blocks))
    ref = tr.compare_report(da, db, tol, row0=owned(ta, blocks)[0])
    bad = ref.pop("bad")
    fb = (got.pop("first_bad_s"), got.pop("first_bad_t"))
    assert got == ref, (got, ref)
    assert (fb in bad) if bad else fb == (-1, -1), (fb, sorted(bad)[:5])
    return got, fb


def apply_kind(kind, a, b, s, t, n):
    """One difference between tables a and b at entry (s, t) (both routable there)."""
    if kind == "lat_ulp":
        a["lat"][s, t] = np.nextafter(b["lat"][s, t], np.inf)
    elif kind == "lat_1e-9":
        a["lat"][s, t] = b["lat"][s, t] * (1 + 1e-9)
    elif kind == "rel_ulp":
        a["rel"][s, t] = np.nextafter(b["rel"][s, t], np.inf)
    elif kind == "rel_1e-9":
        a["rel"][s, t] = b["rel"][s, t] * (1 - 1e-9)
    elif kind == "next":
        a["next"][s, t] = (b["next"][s, t] + 1) % n
    elif kind == "hops":
        a["hops"][s, t] = b["hops"][s, t] + 1
    elif kind == "hops40000_both":
        a["hops"][s, t] = b["hops"][s, t] = 40000
    elif kind == "hops40000_a":
        a["hops"][s, t] = 40000
    elif kind in ("unroutable_a", "unroutable_b"):
        for k, v in UNROUTABLE.items():
            (a if kind == "unroutable_a" else b)[k][s, t] = v
    elif kind == "flip":       # ceil(lat * 1e6): 500001 against 500000, 2.2e-16 apart
        b["lat"][s, t] = 0.5
        a["lat"][s, t] = np.nextafter(0.5, 1.0)
    else:
        raise ValueError(kind)


# what each kind must report besides equalling the reference ("bad": first_bad is that pair)
KINDS = {
    "lat_ulp": dict(latency_differs=1, reliability_differs=0, beyond_tolerance=0, route_mismatch=0),
    "lat_1e-9": dict(latency_differs=1, beyond_tolerance=1, route_mismatch=0, bad=True),
    "rel_ulp": dict(reliability_differs=1, latency_differs=0, beyond_tolerance=0, route_mismatch=0),
    "rel_1e-9": dict(reliability_differs=1, beyond_tolerance=1, route_mismatch=0, bad=True),
    "next": dict(route_mismatch=1, latency_differs=0, beyond_tolerance=0, bad=True),
    "hops": dict(route_mismatch=1, latency_differs=0, beyond_tolerance=0, bad=True),
    "hops40000_both": dict(route_mismatch=0, latency_differs=0, reliability_differs=0, delivery_flips=0),
    "hops40000_a": dict(route_mismatch=1, bad=True),
    "unroutable_a": dict(route_mismatch=1, routable=300 * 300, latency_differs=0, delivery_flips=0, bad=True),
    "unroutable_b": dict(route_mismatch=1, routable=300 * 300 - 1, latency_differs=0, delivery_flips=0, bad=True),
    "flip": dict(delivery_flips=1, latency_differs=1, beyond_tolerance=0, route_mismatch=0),
}
POSITIONS = [(0, 0), (63, 299), (256, 0), (299, 299)]   # first entry; lane 63 of block 0; lane 0 of the last block; last


def test_compare_identical_clones(spe, torch, R):
    a = adopt(spe, R.g, R.att, clone(torch, R.bufs))
    got, fb = assert_compare(a, R.table)
    assert got == dict(pairs=300 * 300, routable=int((R.rows["lat"] > -1.0).sum()), route_mismatch=0,
                       latency_differs=0, reliability_differs=0, beyond_tolerance=0, delivery_flips=0,
                       max_latency_rel_err=0.0, max_reliability_rel_err=0.0)
    assert fb == (-1, -1)


@pytest.mark.parametrize("kind", list(KINDS))
def test_compare_one_difference(spe, torch, R, kind):
    for s, t in POSITIONS:
        a, b = copy_rows(R.rows), copy_rows(R.rows)
        apply_kind(kind, a, b, s, t, R.top.n)
        ta, tb = perturbed(spe, torch, R, a), perturbed(spe, torch, R, b)
        got, fb = assert_compare(ta, tb)
        exp = dict(KINDS[kind])
        if exp.pop("bad", False):
            assert fb == (s, t)
        else:
            assert fb == (-1, -1)
        assert got["pairs"] == 300 * 300
        for k, v in exp.items():
            assert got[k] == v, (kind, (s, t), k, got)


def test_compare_tolerance_is_relative_to_b(spe, torch, R):
    one, two = copy_rows(R.rows), copy_rows(R.rows)
    one["lat"][70, 7], two["lat"][70, 7] = 1.0, 2.0
    one["rel"][299, 0], two["rel"][299, 0] = 0.25, 1.0
    t1, t2 = perturbed(spe, torch, R, one), perturbed(spe, torch, R, two)
    got, _ = assert_compare(t1, t2)
    assert got["max_latency_rel_err"] == 0.5 and got["max_reliability_rel_err"] == 0.75
    got, _ = assert_compare(t2, t1)
    assert got["max_latency_rel_err"] == 1.0 and got["max_reliability_rel_err"] == 3.0
    # the tolerance is applied the same way round: 0.5 passes 0.6, 1.0 does not
    assert t1.compare(t2, 0.8)["beyond_tolerance"] == 0
    assert t2.compare(t1, 0.8)["beyond_tolerance"] == 2


def test_compare_ignores_padding_lanes(spe, torch, R):
    bufs = clone(torch, R.bufs)
    fill_padding(torch, bufs, R.A, 0, 5, 5)
    a = adopt(spe, R.g, R.att, bufs)
    clean, _ = assert_compare(adopt(spe, R.g, R.att, clone(torch, R.bufs)), R.table)
    for x, y in ((a, R.table), (R.table, a)):
        got, fb = assert_compare(x, y)
        assert got == clean and fb == (-1, -1)


def mixed_compare_tables(R, count, seed, rows0=0, rows1=None):
    rng = np.random.default_rng(seed)
    rows1 = R.A if rows1 is None else rows1
    a, b = copy_rows(R.rows), copy_rows(R.rows)
    kinds = list(KINDS)
    for e in rng.choice((rows1 - rows0) * R.A, count, replace=False):
        apply_kind(kinds[rng.integers(len(kinds))], a, b, rows0 + int(e) // R.A, int(e) % R.A, R.top.n)
    return a, b


def test_compare_mixed_perturbations(spe, torch, R):
    a, b = mixed_compare_tables(R, 1000, 17)
    ta, tb = perturbed(spe, torch, R, a), perturbed(spe, torch, R, b)
    got, fb = assert_compare(ta, tb)
    assert got["route_mismatch"] > 300 and got["beyond_tolerance"] > 100 and got["delivery_flips"] > 50
    assert got["routable"] < 300 * 300 and fb != (-1, -1)
    assert_compare(tb, ta)
    assert_compare(ta, tb, tol=1e-8)


@pytest.mark.parametrize("blocks", [(1, 4), (3, 5)])
def test_compare_block_range_tables(spe, torch, R, blocks):
    b0, b1 = blocks
    r0, r1 = tr.owned_rows(R.A, b0, b1)
    built = spe.PathTable(R.g, R.att, blocks=blocks, exact_sources=True)
    built.build()
    same = perturbed(spe, torch, R, R.rows, blocks)     # a slice of R's own content
    got, fb = assert_compare(same, built, blocks=blocks)
    assert got["pairs"] == (r1 - r0) * R.A and got["routable"] == got["pairs"] and fb == (-1, -1)
    assert got["route_mismatch"] == got["latency_differs"] == got["reliability_differs"] == 0
    # one perturbed entry: reported with its absolute slot
    for s, t in ((r0, 5), (r1 - 1, R.A - 1), (r0 + 64, 0)):
        a = copy_rows(R.rows)
        a["hops"][s, t] += 1
        a["hops"][0, 0] += 1 if b0 > 0 else 0             # outside the owned blocks: not in the slice
        got, fb = assert_compare(perturbed(spe, torch, R, a, blocks), built, blocks=blocks)
        assert got["route_mismatch"] == 1 and fb == (s, t)
    # many, with garbage in the padding lanes where the range has them
    a, b = mixed_compare_tables(R, 400, 23 + b0, r0, r1)
    ta, tb = perturbed(spe, torch, R, a, blocks), perturbed(spe, torch, R, b, blocks)
    if b1 == 5:
        fill_padding(torch, ta._bufs, R.A, b0, b1, 3)
    got, fb = assert_compare(ta, tb, blocks=blocks)
    assert got["pairs"] == (r1 - r0) * R.A and got["route_mismatch"] > 100 and r0 <= fb[0] < r1


def test_compare_refusals(spe, torch, R):
    whole = adopt(spe, R.g, R.att, R.bufs)
    e0, e1 = 1 * R.A * 64, 4 * R.A * 64
    part = adopt(spe, R.g, R.att, [b[e0:e1] for b in R.bufs], blocks=(1, 4))
    other = adopt(spe, R.g, R.att, [b[e0:] for b in R.bufs], blocks=(1, 5))
    fewer = adopt(spe, R.g, R.att[:200], R.bufs)                                 # 4 x 200 x 64 elements: fits
    order = adopt(spe, R.g, np.ascontiguousarray(R.att[::-1]), R.bufs)
    unbuilt = spe.PathTable(R.g, R.att, exact_sources=True)
    for a, b in ((whole, part), (part, other), (whole, fewer), (whole, order), (whole, unbuilt), (unbuilt, whole)):
        with pytest.raises(spe.SpeError):
            a.compare(b)
    assert whole.compare(R.table)["pairs"] == 300 * 300   # and the same call on comparable tables goes through


# ---- grid-stride tails: a table larger than one pass of the capped grids ----------------------

class Big:
    A = 2100                    # 33 blocks x 2100 x 64 = 4,435,200 elements


@pytest.fixture(scope="module")
def big(spe, torch):
    """Index-encoded synthetic content (no build): latency s * A + t + 0.5."""
    b = Big()
    A = b.A
    assert tr.nblocks(A) * A * 64 - GRID_CAP == 240896
    b.att = np.arange(A, dtype=np.int32)
    b.g = spe.Graph(ring(A))
    s, t = np.meshgrid(np.arange(A, dtype=np.int64), np.arange(A, dtype=np.int64), indexing="ij")
    b.rows = {"lat": s * A + t + 0.5, "rel": (1.0 + s * A + t) / (A * A + 1.0), "next": ((s + t) % A).astype(np.int32),
              "hops": (1 + (s * 7 + t) % 50000).astype(np.int32)}
    b.bufs = upload(torch, b.rows, A, 0, 33)
    b.table = adopt(spe, b.g, b.att, b.bufs)
    return b


# entries of the second grid-stride pass only: (s, t, kind)
TAIL = [(1984, 436, "lat_1e-9"),      # element 16384 * 256 exactly: the first of the second pass
        (1989, 436, "lat_ulp"), (2047, 2099, "rel_ulp"), (2000, 1000, "rel_1e-9"), (2048, 0, "next"),
        (2048, 1, "hops"), (2060, 2000, "hops40000_a"), (2098, 3, "unroutable_a"), (2099, 2098, "unroutable_b"),
        (2050, 77, "flip"), (2099, 2099, "hops")]   # ... and the table's last real entry


def test_compare_counts_the_second_grid_stride_pass(spe, torch, big):
    A = big.A
    a, b = copy_rows(big.rows), copy_rows(big.rows)
    for s, t, kind in TAIL:
        assert tr.sb64_offset(A, 0, s, t) >= GRID_CAP
        apply_kind(kind, a, b, s, t, A)
    assert tr.sb64_offset(A, 0, *TAIL[0][:2]) == GRID_CAP
    bufs_a, bufs_b = clone(torch, big.bufs), clone(torch, big.bufs)
    assert push(torch, bufs_a, a, big.rows, A) == 10 and push(torch, bufs_b, b, big.rows, A) == 2
    ta, tb = adopt(spe, big.g, big.att, bufs_a), adopt(spe, big.g, big.att, bufs_b)
    got, fb = assert_compare(ta, tb, rows=(a, b))
    assert got == dict(pairs=A * A, routable=A * A - 1, route_mismatch=6, latency_differs=3, reliability_differs=2,
                       beyond_tolerance=2, delivery_flips=got["delivery_flips"],
                       max_latency_rel_err=got["max_latency_rel_err"],
                       max_reliability_rel_err=got["max_reliability_rel_err"])
    assert got["delivery_flips"] >= 2      # the flip entry and the 1e-9 one (4.2e6 ms x 1e-9 x 1e6 > 1)
    assert 0.9e-9 < got["max_latency_rel_err"] < 1.1e-9 and 0.9e-9 < got["max_reliability_rel_err"] < 1.1e-9
    # the download of such a table is what was uploaded (33 blocks: the piped path)
    d = download(ta)
    for k in tr.FIELDS:
        assert d[k].tobytes() == a[k].tobytes(), k


def test_min_latency_beyond_its_grid_cap(spe, torch, big):
    A = big.A
    assert big.table.min_latency() == 0.5
    bufs = clone(torch, big.bufs)
    t = adopt(spe, big.g, big.att, bufs)
    pm = torch.from_numpy(tr.padding_mask(A, 0, 33)).cuda()
    bufs[0][:, 0] += 10.0                                  # every latency 10.5 or more ...
    bufs[0][pm, 0] = -1.0                                  # ... the padding lanes as they were
    o = int(tr.sb64_offset(A, 0, 2099, 7))
    assert o >= 4 * MIN_CAP                                # the fifth pass of k_min_latency's grid
    bufs[0][o, 0] = 0.25
    torch.cuda.synchronize()
    assert t.min_latency() == 0.25
    # an unroutable entry and a smaller latency in a padding lane (slot 2100 of block 32) are no minimum
    bufs[0][int(tr.sb64_offset(A, 0, 2099, 8)), 0] = -1.0
    p = (32 * A + 9) * 64 + (2100 - 2048)
    assert bool(pm[p])
    bufs[0][p, 0] = 0.125
    torch.cuda.synchronize()
    assert t.min_latency() == 0.25


def test_lookup_batch_beyond_its_grid_cap(spe, torch, big):
    A = big.A
    q = GRID_CAP + 1000
    gen = torch.Generator(device="cuda").manual_seed(5)
    pairs = torch.randint(0, A, (q, 2), dtype=torch.int32, device="cuda", generator=gen)
    pairs[-1, 0], pairs[-1, 1] = A - 1, A - 1
    lat = torch.full((q,), -7.0, dtype=torch.float64, device="cuda")
    rel = torch.full((q,), -7.0, dtype=torch.float64, device="cuda")
    ok = torch.full((q,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    big.table.lookup_batch(pairs.data_ptr(), q, lat.data_ptr(), rel.data_ptr(), ok.data_ptr())
    torch.cuda.synchronize()
    p = pairs.cpu().numpy().astype(np.int64)
    idx = p[:, 0] * A + p[:, 1]          # the encoding of big.rows, in numpy as there (IEEE division)
    lat, rel, ok = lat.cpu().numpy(), rel.cpu().numpy(), ok.cpu().numpy()
    for name, sl in (("first pass", slice(0, GRID_CAP)), ("second pass", slice(GRID_CAP, q))):
        assert np.array_equal(lat[sl], idx[sl] + 0.5), name
        assert np.array_equal(rel[sl], (1.0 + idx[sl]) / (A * A + 1.0)), name
        assert (ok[sl] == 1).all(), name


# ---- spe_table_check -------------------------------------------------------------------------

def assert_check(t, top, att, rows=None):
    got = t.check()
    ref = tr.check_report(top, att, rows or download(t))
    bad = ref.pop("bad")
    fb = (got.pop("first_bad_s"), got.pop("first_bad_t"))
    assert got == ref, (got, ref)
    assert (fb in bad) if bad else fb == (-1, -1), (fb, sorted(bad)[:5])
    return got


def two_components():
    a, b = graphs.gen_random_small(150, 300, 71), graphs.gen_random_small(150, 300, 72)
    return Topology(n=300, esrc=np.concatenate([a.esrc, b.esrc + 150]).astype(np.int32),
                    edst=np.concatenate([a.edst, b.edst + 150]).astype(np.int32), elat=np.concatenate([a.elat, b.elat]),
                    eloss=np.concatenate([a.eloss, b.eloss]), vloss=np.concatenate([a.vloss, b.vloss]))


def test_check_unperturbed_tables(spe, R):
    A = R.A
    got = assert_check(R.table, R.top, R.att, R.rows)
    assert got["pairs"] == A * (A - 1) == got["sym_checked"] and got["unroutable"] == 0
    assert got["bad_values"] == got["next_not_adjacent"] == got["hop_mismatch"] == got["sym_mismatch"] == 0
    assert 0 < got["hop_checked"] < got["pairs"]

    top = graphs.gen_random_small(300, 900, 62, directed=True)
    t = spe.PathTable(spe.Graph(top), R.att, exact_sources=True)
    t.build()
    got = assert_check(t, top, R.att)
    assert got["sym_checked"] == 0 and got["pairs"] == A * (A - 1) and got["hop_checked"] > 0
    assert got["bad_values"] == got["next_not_adjacent"] == got["hop_mismatch"] == 0

    top = graphs.gen_random_small(600, 1800, 63)
    att = np.sort(np.random.default_rng(63).choice(600, 100, replace=False)).astype(np.int32)
    t = spe.PathTable(spe.Graph(top), att, exact_sources=True)
    t.build()
    got = assert_check(t, top, att)
    assert got["pairs"] == 100 * 99 and 0 < got["hop_checked"] < got["pairs"]
    assert got["bad_values"] == got["next_not_adjacent"] == got["hop_mismatch"] == got["sym_mismatch"] == 0

    top = two_components()
    t = spe.PathTable(spe.Graph(top), R.att, exact_sources=True)
    t.build()
    got = assert_check(t, top, R.att)
    assert got["unroutable"] == 2 * 150 * 150 and got["pairs"] == A * (A - 1)
    assert got["bad_values"] == got["next_not_adjacent"] == got["hop_mismatch"] == 0


def neighbours(top, v):
    """Vertices with an edge v -> u (either direction: undirected), v itself left out."""
    u = np.concatenate([top.edst[top.esrc == v], top.esrc[top.edst == v]])
    return sorted(set(u.tolist()) - {v})


def apply_check_kind(kind, rows, R, s, t):
    """One violation at entry (s, t), s != t, of R's table (slots = vertices)."""
    nb = neighbours(R.top, s)
    if kind == "next_non_neighbour":
        rows["next"][s, t] = next(v for v in range(R.top.n) if v != s and v not in nb)
    elif kind == "next_other_neighbour":
        rows["next"][s, t] = next(v for v in nb if v != rows["next"][s, t])
    elif kind == "hops":
        rows["hops"][s, t] += 1
    elif kind == "lat_1e-9":
        rows["lat"][s, t] *= 1 + 1e-9
    elif kind == "lat_0":
        rows["lat"][s, t] = 0.0
    elif kind == "rel_1.5":
        rows["rel"][s, t] = 1.5
    elif kind == "rel_0":
        rows["rel"][s, t] = 0.0
    elif kind == "hops_0":
        rows["hops"][s, t] = 0
    elif kind == "next_n":
        rows["next"][s, t] = R.top.n
    else:
        raise ValueError(kind)


CHECK_KINDS = ["next_non_neighbour", "next_other_neighbour", "hops", "lat_1e-9", "lat_0", "rel_1.5", "rel_0", "hops_0",
               "next_n"]
CHECK_POSITIONS = [(0, 1), (63, 299), (256, 0), (299, 298)]


def with_two_neighbours(R, s, t):
    while len(neighbours(R.top, s)) < 2 or s == t:
        s = (s + 1) % R.A
    return s


@pytest.mark.parametrize("kind", CHECK_KINDS)
def test_check_one_violation(spe, torch, R, kind):
    clean = tr.check_report(R.top, R.att, R.rows)
    hop_mismatches = 0
    for s, t in CHECK_POSITIONS:
        if kind == "next_other_neighbour":
            s = with_two_neighbours(R, s, t)
        rows = copy_rows(R.rows)
        apply_check_kind(kind, rows, R, s, t)
        got = assert_check(perturbed(spe, torch, R, rows), R.top, R.att)
        moved = {k for k in got if got[k] != clean[k]}
        if kind == "next_non_neighbour":
            assert got["next_not_adjacent"] == 1 and moved <= {"next_not_adjacent", "hop_checked", "hop_mismatch"}
        elif kind == "next_other_neighbour":   # adjacent: only the hop rule can tell
            assert got["next_not_adjacent"] == 0 and moved <= {"hop_checked", "hop_mismatch"}
        elif kind == "hops":                   # the entry itself and / or the entries whose rule reads it
            assert moved <= {"hop_mismatch"}
            hop_mismatches += got["hop_mismatch"]
        elif kind == "lat_1e-9":
            d = rows["lat"][s, t] - R.rows["lat"][t, s]
            assert got["sym_mismatch"] == 2 and moved == {"sym_mismatch", "max_sym_rel_err"}
            assert got["max_sym_rel_err"] == max(abs(d) / rows["lat"][s, t], abs(d) / R.rows["lat"][t, s])
        else:   # bad values: that entry takes no further check; (t, s) still compares itself with it
            assert got["bad_values"] == 1 and got["next_not_adjacent"] == 0
            assert got["sym_checked"] == clean["sym_checked"] - 1
            assert got["sym_mismatch"] == (1 if kind in ("lat_0", "rel_1.5", "rel_0") else 0)
            # hops = 0 is also read by the hop rule of the entries that go through s to t
            assert got["hop_mismatch"] == 0 or kind == "hops_0"
            assert moved <= {"bad_values", "hop_checked", "hop_mismatch", "sym_checked", "sym_mismatch", "max_sym_rel_err"}
    if kind == "hops":
        assert hop_mismatches >= 1


def test_check_mixed_violations_and_padding(spe, torch, R):
    rng = np.random.default_rng(29)
    rows = copy_rows(R.rows)
    n = 0
    for e in rng.choice(R.A * R.A, 230, replace=False):
        s, t = int(e) // R.A, int(e) % R.A
        kind = CHECK_KINDS[rng.integers(len(CHECK_KINDS))]
        if s == t or (kind == "next_other_neighbour" and len(neighbours(R.top, s)) < 2):
            continue
        apply_check_kind(kind, rows, R, s, t)
        n += 1
    assert n >= 200
    t = perturbed(spe, torch, R, rows)
    got = assert_check(t, R.top, R.att)
    assert got["bad_values"] > 50 and got["next_not_adjacent"] > 10 and got["hop_mismatch"] > 20 and got["sym_mismatch"] > 50
    # garbage in the padding lanes changes neither this report nor the clean one
    fill_padding(torch, t._bufs, R.A, 0, 5, 7)
    assert assert_check(t, R.top, R.att) == got
    bufs = clone(torch, R.bufs)
    fill_padding(torch, bufs, R.A, 0, 5, 8)
    clean = assert_check(R.table, R.top, R.att, R.rows)
    assert assert_check(adopt(spe, R.g, R.att, bufs), R.top, R.att) == clean


# ---- lookups, downloads and row reads on index-encoded tables ----------------------------------

def encoded_rows(A, unroutable=()):
    """Every entry and field distinct; hops run past 32768."""
    s, t = np.meshgrid(np.arange(A, dtype=np.int64), np.arange(A, dtype=np.int64), indexing="ij")
    rows = {"lat": s * A + t + 0.5, "rel": (1.0 + s * A + t) / (A * A + 1.0), "next": (s * A + t).astype(np.int32),
            "hops": ((s * A + t) % 65536).astype(np.int32)}
    for s_, t_ in unroutable:
        for k, v in UNROUTABLE.items():
            rows[k][s_, t_] = v
    return rows


class Enc:
    pass


ENC = {"A300": (300, None), "A300-blocks1-4": (300, (1, 4)), "A450": (450, None), "A450-blocks1-7": (450, (1, 7))}


@pytest.fixture(scope="module")
def enc_tables(spe, torch):
    """Index-encoded tables by name, each made once: whole or a block range; the
    padding lanes (the last block of the whole tables: 300 = 4 x 64 + 44,
    450 = 7 x 64 + 2) hold positive latencies.  A = 450 is there for the row
    range [130, 389), which A = 300 has no rows for."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_enc(spe, torch, *ENC[name])
        return made[name]
    return get


def make_enc(spe, torch, A, blocks):
    e = Enc()
    e.A, e.blocks = A, blocks
    e.b0, e.b1 = e.blocks or (0, tr.nblocks(e.A))
    e.r0, e.r1 = tr.owned_rows(e.A, e.b0, e.b1)
    full = encoded_rows(e.A, unroutable=[(0, 0), (70, 5), (255, e.A - 1), (e.A - 1, e.A - 1), (100, 100)])
    e.rows = {k: v[e.r0:e.r1] for k, v in full.items()}
    e.att = np.arange(e.A, dtype=np.int32)
    e.g = spe.Graph(ring(e.A))
    e.bufs = upload(torch, e.rows, e.A, e.b0, e.b1, pad=garbage_pad(e.A, e.b0, e.b1, 11))
    if e.blocks is None:
        pm = tr.padding_mask(e.A, e.b0, e.b1)
        lr = e.bufs[0].cpu().numpy()
        assert pm.any() and (lr[pm, 0] > 0).sum() > 0.5 * pm.sum()    # a lookup answered from there says ok = 1
    e.table = adopt(spe, e.g, e.att, e.bufs, e.blocks)
    return e


def lookup_pairs(A, seed=0, random=10000):
    S = [-1, 0, 63, 64, 255, 256, A - 1, A, A + 1, 64 * tr.nblocks(A) - 1, 64 * tr.nblocks(A), 2**31 - 1]
    T = [-1, 0, A - 1, A, 2**31 - 1]
    edge = np.array([(s, t) for s in S for t in T], np.int64)
    rnd = np.random.default_rng(seed).integers(0, A, (random, 2))
    return np.concatenate([edge, rnd, [(0, 0), (70, 5)]]).astype(np.int32)     # ... and two unroutable entries


def assert_lookup(got, exp, pairs):
    for name, g, x in zip(("latency", "reliability", "ok"), got, exp):
        bad = np.nonzero(~((g == x) | ((g != g) & (x != x))))[0]
        assert bad.size == 0, (f"{name}: {bad.size} of {len(pairs)} pairs differ, first (s, t) = "
                               f"{pairs[bad[:8]].tolist()}: got {g[bad[:8]].tolist()}, expected {x[bad[:8]].tolist()}")


@pytest.mark.parametrize("name", list(ENC))
def test_lookup_batch_refuses_every_slot_that_is_not_attached(spe, torch, enc_tables, name):
    """Pairs outside [0, A) x [0, A) or in a block the table does not own return
    (-1, -1, ok 0) -- also a source slot in the padding lanes of the last block,
    A <= s < 64 * ceil(A / 64), whatever those lanes hold."""
    enc = enc_tables(name)
    pairs = lookup_pairs(enc.A)
    exp = tr.lookup_answers(enc.rows["lat"], enc.rows["rel"], enc.A, enc.b0, enc.b1, pairs)
    assert exp[2].sum() > 2000 and (exp[2] == 0).sum() > 40
    q = len(pairs)
    d_pairs = torch.from_numpy(pairs).cuda()
    lat = torch.full((q,), -7.0, dtype=torch.float64, device="cuda")
    rel = torch.full((q,), -7.0, dtype=torch.float64, device="cuda")
    ok = torch.full((q,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    enc.table.lookup_batch(d_pairs.data_ptr(), q, lat.data_ptr(), rel.data_ptr(), ok.data_ptr())
    torch.cuda.synchronize()
    assert_lookup((lat.cpu().numpy(), rel.cpu().numpy(), ok.cpu().numpy()), exp, pairs)
    assert_lookup(enc.table.lookup_batch_host(pairs), exp, pairs)


@pytest.mark.parametrize("name", ["A300", "A300-blocks1-4"])
def test_lookup_batch_host_three_chunks(spe, enc_tables, name):
    """q = 2 * 2^21 + 77: three chunks of the host call, the last ragged, both
    staging slots reused."""
    enc = enc_tables(name)
    base = lookup_pairs(enc.A, seed=1)
    q = 2 * 2**21 + 77
    pairs = base[np.random.default_rng(2).integers(0, len(base), q)]
    pairs[-77:] = base[:77]          # the ragged chunk holds the edge cases
    exp = tr.lookup_answers(enc.rows["lat"], enc.rows["rel"], enc.A, enc.b0, enc.b1, pairs)
    assert_lookup(enc.table.lookup_batch_host(pairs), exp, pairs)


def row_ranges(e):
    """Row ranges of the issue's list, moved into the owned rows [r0, r1): whole,
    unaligned, one row either side of a block boundary, the last row, five blocks
    unaligned at both ends (the piped path, where the table has them), empty."""
    r0, r1 = e.r0, e.r1
    rr = [(r0, r1), (r0 + 5, r0 + 70), (r0 + 63, r0 + 64), (r0 + 64, r0 + 65), (r1 - 1, r1), (r0 + 7, r0 + 7)]
    if r1 - r0 > 4 * 64:
        rr.append((130, 389) if r1 >= 389 else (r0 + 2, r1 - 3))
        assert tr.nblocks(rr[-1][1]) - rr[-1][0] // 64 >= 5
    return rr


@pytest.mark.parametrize("name", list(ENC))
def test_download_ranges_and_field_subsets(spe, enc_tables, name):
    """Every row range x field subset equals what was uploaded, bit for bit: the
    single-slot and the piped path of download_rows, the staging tiles k_sb64_rows
    shares between fields, hops >= 32768."""
    enc = enc_tables(name)
    assert (enc.rows["hops"] >= 32768).any()
    for a, b in row_ranges(enc):
        for fields in (tr.FIELDS, ("next",), ("hops",), ("rel",), ("lat",)):
            d = enc.table.download(a, b, fields=fields)
            assert set(d) - {"ok"} == set(fields)
            for k in fields:
                exp = enc.rows[k][a - enc.r0:b - enc.r0]
                assert d[k].shape == exp.shape and d[k].tobytes() == np.ascontiguousarray(exp, d[k].dtype).tobytes(), \
                    ((a, b), fields, k)
    for a, b in ((enc.r0 - 1, enc.r0 + 1), (enc.r1 - 1, enc.r1 + 1), (enc.A, enc.A + 1)):
        if a >= 0:
            with pytest.raises(spe.SpeError):
                enc.table.download(a, b)


@pytest.mark.parametrize("name", list(ENC))
def test_get_row_latrel(spe, enc_tables, name):
    enc = enc_tables(name)
    for s in sorted({enc.r0, enc.r0 + 63, enc.r0 + 64, enc.r1 - 1}):
        lat, rel = enc.table.get_row_latrel(s)
        assert lat.tobytes() == enc.rows["lat"][s - enc.r0].tobytes(), s
        assert rel.tobytes() == enc.rows["rel"][s - enc.r0].tobytes(), s
    for s in (-1, enc.A, enc.r0 - 1 if enc.r0 else enc.A + 5, enc.r1 if enc.r1 < enc.A else 64 * tr.nblocks(enc.A) - 1):
        with pytest.raises(spe.SpeError):
            enc.table.get_row_latrel(s)
