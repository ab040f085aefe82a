"""spe_table_digest / spe_table_digest_replica / spe_table_verify_replicas on the device
against the numpy restatement of the digest (tests/table_digest.py, checked by hand in
test_table_digest.py).

Hand-laid tables live in torch buffers adopted with ext_filled (as in
test_gpu_table_reports.py), so a test writes any SB64 content -- garbage in the padding
lanes included -- and predicts every digest with numpy.  Built tables are digested
against the mirror's digests of their download; multi-device tables (three replicas on
the one GPU) against a single-device build, before and after one record of one replica is
overwritten through spe_table_replica_latrel."""
import ctypes

import numpy as np
import pytest

import table_digest as td
import table_reports as tr
from shadow_amd import graphs
from shadow_amd.graphs import Topology

pytestmark = [pytest.mark.gpu, pytest.mark.engine_fixed]

DG_TC = 128                     # targets per work item of k_table_digest (one wave per item)
DG_WAVES = 2048 * 4             # waves of its capped grid: items beyond take a second grid-stride pass
ENGINES = {"batch": 1, "lds": 2, "fw": 3}


@pytest.fixture(scope="module")
def spe():
    from shadow_amd import spe as m
    assert m.device_count() > 0, "no GPU visible"
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as m
    return m


def ring(n):
    """Any valid graph over n vertices, for tables whose content is synthetic."""
    v = np.arange(n, dtype=np.int32)
    return Topology(n=n, esrc=v, edst=((v + 1) % n).astype(np.int32), elat=np.full(n, 1.0), eloss=np.zeros(n),
                    vloss=np.zeros(n))


def garbage(A, b0, b1, seed):
    """Span-shaped content for the padding lanes that would count if it were read."""
    rng = np.random.default_rng(seed)
    e = (b1 - b0) * A * tr.WAVE
    return {"lr": rng.uniform(1e-3, 40.0, (e, 2)), "next": rng.integers(-5, 10**6, e).astype(np.int32),
            "hops": rng.integers(-32768, 32768, e).astype(np.int16)}


def upload(torch, rows, A, b0, b1, pad):
    """Row-major owned rows -> the three SB64 device tensors, padding lanes from `pad`."""
    lr = tr.pack_sb64(np.stack([rows["lat"], rows["rel"]], -1), A, b0, b1, pad["lr"])
    nx = tr.pack_sb64(np.asarray(rows["next"], np.int32), A, b0, b1, pad["next"])
    hp = tr.pack_sb64(tr.hops_to_i16(rows["hops"]), A, b0, b1, pad["hops"])
    bufs = [torch.from_numpy(x).cuda() for x in (lr, nx, hp)]
    torch.cuda.synchronize()
    return bufs


def adopt(spe, g, attached, bufs, blocks=None):
    t = spe.PathTable(g, attached, ext=[b.data_ptr() for b in bufs], ext_filled=True, blocks=blocks)
    t._bufs = bufs   # the storage outlives the table
    return t


def assert_digests(got, want, what=""):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: (block, field) {bad[:8].tolist()} differ: got {got[got != want][:8]}, " \
                          f"mirror {want[got != want][:8]}"


# ---- A = 130: three blocks, the last with 2 real and 62 padding lanes ---------------------------

class T130:
    A = 130


@pytest.fixture(scope="module")
def small(spe, torch):
    s = T130()
    s.att = np.arange(s.A, dtype=np.int32)
    s.g = spe.Graph(ring(s.A))
    s.rows = td.seeded_rows(s.A, 11)
    s.bufs = upload(torch, s.rows, s.A, 0, 3, garbage(s.A, 0, 3, 12))
    pm = tr.padding_mask(s.A, 0, 3)
    assert pm.sum() == 62 * s.A
    s.table = adopt(spe, s.g, s.att, s.bufs)
    s.want = td.block_digests(s.rows, s.A, 0, 3)
    return s


def test_a130_every_block_and_field_equals_the_mirror(small):
    got = small.table.digest()
    assert_digests(got, small.want, "A = 130")
    assert len(set(got.ravel().tolist())) == 12           # twelve different sums, none 0
    again = small.table.digest()
    assert again.tobytes() == got.tobytes()               # deterministic: the same bits twice
    for b0, b1 in ((0, 1), (1, 3), (2, 3)):               # sub-ranges of the owned blocks
        assert_digests(small.table.digest(b0, b1), small.want[b0:b1], f"blocks {b0}:{b1}")


def test_a130_table_owning_blocks_1_to_3(spe, small):
    e0 = 1 * small.A * 64
    part = adopt(spe, small.g, small.att, [b[e0:] for b in small.bufs], blocks=(1, 3))
    assert_digests(part.digest(), small.want[1:3], "blocks (1, 3)")
    assert_digests(part.digest(2, 3), small.want[2:3], "block 2 of (1, 3)")
    assert_digests(part.digest(replica=0), small.want[1:3], "replica 0 of a single-device table")


def change(rows, field, s, t):
    if field in ("lat", "rel"):
        rows[field][s, t] = np.nextafter(rows[field][s, t], np.inf)      # one ulp (the unroutable -1 too)
    elif field == "next":
        rows[field][s, t] = -1 if rows[field][s, t] != -1 else 0
    else:
        rows[field][s, t] = rows[field][s, t] ^ 0x8000                    # across the int16 sign bit


@pytest.mark.parametrize("field", td.FIELDS)
def test_one_change_per_field(spe, torch, small, field):
    A = small.A
    f = td.FIELDS.index(field)
    bufs = [b.clone() for b in small.bufs]
    t = adopt(spe, small.g, small.att, bufs)
    for s, tt in ((0, 0), (63, A - 1), (64, 0), (129, A - 1)):
        rows = {k: np.array(v) for k, v in small.rows.items()}
        change(rows, field, s, tt)
        o = int(tr.sb64_offset(A, 0, s, tt))
        if field == "lat":
            bufs[0][o, 0] = float(rows["lat"][s, tt])
        elif field == "rel":
            bufs[0][o, 1] = float(rows["rel"][s, tt])
        elif field == "next":
            bufs[1][o] = int(rows["next"][s, tt])
        else:
            bufs[2][o] = int(tr.hops_to_i16(rows["hops"][s, tt]))
        torch.cuda.synchronize()
        got = t.digest()
        want = td.block_digests(rows, A, 0, 3)
        moved = np.argwhere(want != small.want).tolist()
        assert moved == [[s // 64, f]]                     # the mirror: exactly that (block, field)
        assert_digests(got, want, f"{field} at {(s, tt)}")
        for b, src in zip(bufs, small.bufs):               # back to the base content
            b.copy_(src)
        torch.cuda.synchronize()
    assert_digests(t.digest(), small.want, "restored")


def test_padding_lanes_change_nothing(spe, torch, small):
    A = small.A
    bufs = [b.clone() for b in small.bufs]
    t = adopt(spe, small.g, small.att, bufs)
    pm = torch.from_numpy(tr.padding_mask(A, 0, 3)).cuda()
    other = garbage(A, 0, 3, 13)
    for b, k in zip(bufs, ("lr", "next", "hops")):
        new = torch.from_numpy(other[k]).cuda()
        assert bool((b[pm] != new[pm]).any())
        b[pm] = new[pm]
    bufs[0][pm] = float("nan")                             # ... and NaNs in every padding record
    torch.cuda.synchronize()
    assert_digests(t.digest(), small.want, "other padding garbage")


# ---- larger hand-laid tables --------------------------------------------------------------------

def test_a2100_several_waves_per_block(spe, torch):
    """A = 2100 (33 blocks, the last with 52 real lanes): every block's sum is made of
    ceil(2100 / 128) = 17 waves' atomic adds.  The digest's capped grid (8192 waves) is
    not reached at this size: test_a8193_second_grid_stride_pass."""
    A = 2100
    nb = tr.nblocks(A)
    assert -(-A // DG_TC) == 17 and nb * 17 < DG_WAVES
    s, t = np.meshgrid(np.arange(A, dtype=np.int64), np.arange(A, dtype=np.int64), indexing="ij")
    rows = {"lat": s * A + t + 0.5, "rel": (1.0 + s * A + t) / (A * A + 1.0), "next": ((s + t) % A - 1).astype(np.int32),
            "hops": ((s * 7 + t) % 65536).astype(np.int32)}
    g = spe.Graph(ring(A))
    att = np.arange(A, dtype=np.int32)
    table = adopt(spe, g, att, upload(torch, rows, A, 0, nb, garbage(A, 0, nb, 14)))
    assert_digests(table.digest(), td.block_digests(rows, A, 0, nb), "A = 2100")


def test_a8193_second_grid_stride_pass(spe, torch):
    """The smallest A at which k_table_digest's grid reaches its cap: 129 blocks x 65
    chunks of 128 targets = 8385 work items for 2048 x 4 = 8192 waves (A = 8192 gives
    128 x 64 = 8192 exactly).  The content is laid on the device by formula, straight
    in SB64 order, padding lanes (63 of the last block's 64) included; the mirror
    digests the blocks around the pass boundary (item 8192 = block 126, chunk 2) from
    the same formulas in numpy."""
    A = 8193
    nb = tr.nblocks(A)
    chunks = -(-A // DG_TC)
    assert nb * chunks == 8385 > DG_WAVES and tr.nblocks(A - 1) * (-(-(A - 1) // DG_TC)) == DG_WAVES
    assert DG_WAVES // chunks == 126
    e = torch.arange(nb * A * 64, dtype=torch.int64, device="cuda")
    s = (e // (A * 64)) * 64 + e % 64
    t = (e // 64) % A
    lr = torch.stack([(s * A + t).to(torch.float64) + 0.5, ((s * 31 + t * 17) % 4096).to(torch.float64) / 4096.0], 1)
    nx = ((s + 3 * t) % 100000 - 1).to(torch.int32)
    hp = (s * 5 + t) % 65536
    hp = torch.where(hp >= 32768, hp - 65536, hp).to(torch.int16)  # the uint16's bit pattern
    del e
    torch.cuda.synchronize()
    table = adopt(spe, spe.Graph(ring(A)), np.arange(A, dtype=np.int32), [lr.contiguous(), nx, hp])
    got = table.digest()
    assert got.shape == (nb, 4)
    for b in (0, 64, 125, 126, 127, 128):
        lo, hi = b * 64, min(A, b * 64 + 64)
        sn, tn = np.meshgrid(np.arange(lo, hi, dtype=np.int64), np.arange(A, dtype=np.int64), indexing="ij")
        rows = {"lat": sn * A + tn + 0.5, "rel": ((sn * 31 + tn * 17) % 4096) / 4096.0,
                "next": ((sn + 3 * tn) % 100000 - 1).astype(np.int32), "hops": ((sn * 5 + tn) % 65536).astype(np.int32)}
        assert_digests(got[b:b + 1], td.block_digests(rows, A, b, b + 1), f"A = 8193, block {b}")
    assert np.unique(got).size == got.size                  # no block left at 0 or added twice alike


# ---- built tables ---------------------------------------------------------------------------------

class Built:
    pass


@pytest.fixture(scope="module")
def built(spe):
    """gen_random_small(700, 2100): 11 blocks, the last with 60 real lanes; one
    single-device build per engine, made on first use."""
    b = Built()
    b.top = graphs.gen_random_small(700, 2100, 65)
    b.A = b.top.n
    b.att = np.arange(b.A, dtype=np.int32)
    b.g = spe.Graph(b.top)
    made = {}

    def single(engine):
        if engine not in made:
            t = spe.PathTable(b.g, b.att, engine=engine, exact_sources=True)
            t.build()
            made[engine] = (t, t.digest())
        return made[engine]
    b.single = single
    return b


@pytest.mark.parametrize("engine", list(ENGINES))
def test_built_table_digest_equals_the_mirror_of_its_download(built, engine):
    t, got = built.single(ENGINES[engine])
    d = t.download()
    assert_digests(got, td.block_digests({k: d[k] for k in td.FIELDS}, built.A, 0, t.nblocks), engine)
    st = t.stats()
    assert st["replica_mismatches"] == -1 and st["verify_seconds"] == 0.0     # one device: never checked
    assert t.verify_replicas() == dict(replicas=1, blocks=t.nblocks, mismatching_blocks=0, first_bad_replica=-1,
                                       first_bad_block=-1, seconds=0.0)


# ---- three replicas on one GPU --------------------------------------------------------------------

def device_bytes(torch, ptr, n):
    """n bytes of device memory at `ptr` as a torch uint8 tensor (no copy)."""
    class Span:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return torch.as_tensor(Span(), device="cuda")


def overwrite(torch, ptr, data):
    view = device_bytes(torch, ptr, len(data))
    view.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()


MULTI = {"batch": dict(engine=1, shared_fraction=1.0), "lds": dict(engine=2, shared_fraction=1.0),
         "fw": dict(engine=3, shared_fraction=1.0),
         "batch-local-blocks": dict(engine=1, shared_fraction=0.5, groups=1)}


@pytest.mark.parametrize("name", list(MULTI))
def test_three_replicas_verify_and_digest(spe, torch, built, name):
    opts = MULTI[name]
    _, base = built.single(opts["engine"])
    t = spe.PathTable(built.g, built.att, devices=[0, 0, 0], exact_sources=True, **opts)
    st = t.build()
    nblk = t.nblocks
    assert st["n_devices"] == 3 and st["replica_mismatches"] == -1 and st["verify_seconds"] == 0.0
    if name == "batch-local-blocks":
        assert st["shared_blocks"] == 3 and st["local_blocks"] == nblk - 3
    else:
        assert st["local_blocks"] == 0
    rep = t.verify_replicas()
    assert rep["seconds"] > 0
    assert {k: v for k, v in rep.items() if k != "seconds"} == dict(
        replicas=3, blocks=nblk, mismatching_blocks=0, first_bad_replica=-1, first_bad_block=-1)
    for r in range(3):
        assert_digests(t.digest(replica=r), base, f"{name}: replica {r} against the single-device table")
    assert_digests(t.digest(), base, f"{name}: the home replica")
    assert_digests(t.digest(3, 9, replica=1), base[3:9], f"{name}: blocks 3:9 of replica 1")
    assert t.replica_latrel(0) == t.layout()["latrel"]
    assert len({t.replica_latrel(r) for r in range(3)}) == 3

    # one 16-byte record of replica 2, in block 5 (built by replica 1, or by every replica itself)
    blk, s, tt = 5, 5 * 64 + 7, 11
    ptr = t.replica_latrel(2) + 16 * int(tr.sb64_offset(built.A, 0, s, tt))
    overwrite(torch, ptr, np.array([123.456, 0.5], np.float64).tobytes())
    rep = t.verify_replicas()
    assert (rep["mismatching_blocks"], rep["first_bad_replica"], rep["first_bad_block"]) == (1, 2, blk), rep
    for r in (0, 1):
        assert_digests(t.digest(replica=r), base, f"{name}: replica {r} after replica 2 was damaged")
    moved = np.argwhere(t.digest(replica=2) != base).tolist()
    assert moved == [[blk, 0], [blk, 1]], moved            # the record's two fields; next hop / hops are the owner's


def test_verify_replicas_at_build(spe, built):
    t = spe.PathTable(built.g, built.att, devices=[0, 0, 0], engine=1, exact_sources=True, verify_replicas=True)
    st = t.build()
    assert st["replica_mismatches"] == 0 and st["verify_seconds"] > 0
    assert st["n_devices"] == 3 and st["seconds"] > 0 and st["gather_seconds"] > 0
    plain = spe.PathTable(built.g, built.att, devices=[0, 0, 0], engine=1, exact_sources=True)
    sp = plain.build()
    assert sp["replica_mismatches"] == -1 and sp["verify_seconds"] == 0.0
    for k in ("n_devices", "gather", "shared_blocks", "local_blocks", "relaxed_lanes", "fallback_blocks", "derived_sources"):
        assert sp[k] == st[k], k                       # (relaxation rounds vary from build to build)
    assert_digests(t.digest(), plain.digest(), "verified against plain build")


# ---- refusals -----------------------------------------------------------------------------------------

def refused(spe, code, call):
    with pytest.raises(spe.SpeError) as e:
        call()
    assert f"({code})" in str(e.value), str(e.value)


def test_refusals(spe, small, built):
    EINVAL, ESTATE = -1, -5
    unbuilt = spe.PathTable(small.g, small.att)
    refused(spe, ESTATE, lambda: unbuilt.digest())
    refused(spe, ESTATE, lambda: unbuilt.digest(replica=0))
    refused(spe, ESTATE, lambda: unbuilt.verify_replicas())
    unbuilt3 = spe.PathTable(built.g, built.att, devices=[0, 0, 0], engine=1)
    refused(spe, ESTATE, lambda: unbuilt3.digest())
    refused(spe, ESTATE, lambda: unbuilt3.verify_replicas())
    whole = small.table
    for b0, b1 in ((2, 1), (1, 1), (0, 4), (-1, 2), (3, 4)):          # reversed, empty, past either end
        refused(spe, EINVAL, lambda: whole.digest(b0, b1))
    e0 = 1 * small.A * 64
    part = adopt(spe, small.g, small.att, [b[e0:] for b in small.bufs], blocks=(1, 3))
    for b0, b1 in ((0, 2), (0, 1), (1, 4)):                           # not owned
        refused(spe, EINVAL, lambda: part.digest(b0, b1))
    refused(spe, EINVAL, lambda: whole.digest(replica=1))              # a single-device table has replica 0 only
    refused(spe, EINVAL, lambda: whole.replica_latrel(1))
    three = spe.PathTable(built.g, built.att, devices=[0, 0, 0], engine=1, exact_sources=True)
    three.build()
    for r in (3, -1):
        refused(spe, EINVAL, lambda: three.digest(replica=r))
        refused(spe, EINVAL, lambda: three.replica_latrel(r))
    refused(spe, EINVAL, lambda: three.digest(0, three.nblocks + 1, replica=1))
    # a report struct of another spe.h
    L = spe.lib()
    stale = spe.ReplicaReport()
    stale.struct_size = ctypes.sizeof(spe.ReplicaReport) - 4
    for t in (whole, three):
        assert L.spe_table_verify_replicas(t.h, ctypes.byref(stale)) == EINVAL
        assert b"struct_size" in L.spe_last_error()
    # NULL arguments
    out = np.zeros((3, 4), np.uint64)
    assert L.spe_table_digest(None, 0, 3, out.ctypes.data) == EINVAL
    assert L.spe_table_digest(whole.h, 0, 3, None) == EINVAL
    assert L.spe_table_digest_replica(whole.h, 0, 0, 3, None) == EINVAL
    assert L.spe_table_replica_latrel(whole.h, 0, None) == EINVAL
    assert L.spe_table_verify_replicas(whole.h, None) == EINVAL
    assert_digests(whole.digest(), small.want, "and the table still digests")


# ---- the drop-in's switch -----------------------------------------------------------------------------

@pytest.mark.parametrize("verify", ["1", None])
def test_topology_shim_verifies_its_replicas(tmp_path, monkeypatch, verify):
    """SHADOW_SPE_VERIFY_REPLICAS=1 with a device list (the one GPU twice): the seal
    verifies and says so in one message-level line; unset, no such line."""
    from oracle import Oracle
    from shadow_amd import topology as T
    monkeypatch.setenv("SHADOW_SPE_DEVICES", "0,0")
    if verify:
        monkeypatch.setenv("SHADOW_SPE_VERIFY_REPLICAS", verify)
    else:
        monkeypatch.delenv("SHADOW_SPE_VERIFY_REPLICAS", raising=False)
    t = graphs.gen_random_small(300, 900, 66)
    ips = [f"10.{v // 250}.{v % 250}.{1 + v % 7}" for v in range(t.n)]
    p = tmp_path / "g.graphml"
    graphs.write_graphml(t, str(p), ips=ips)
    top = T.Topology(str(p))
    top.capture_logs(3)                                            # message level
    verts = np.random.default_rng(66).choice(t.n, 150, replace=False).astype(np.int32)
    addrs = [T.ip(f"11.0.0.{i + 1}") for i in range(150)]
    for a, v in zip(addrs, verts):
        top.attach(a, ip_hint=ips[v])
    assert top.seal() == 0
    lines = [text for lvl, text in top.logs if "path table verified" in text]
    if verify:
        assert len(lines) == 1 and "2 replicas of 3 blocks" in lines[0], top.logs[-5:]
    else:
        assert lines == []
    ref = Oracle(t).rows(verts, verts)
    for i in range(0, 150, 15):
        for j in range(0, 150, 10):
            assert top.path_info(addrs[i], addrs[j]) == (True, ref["lat"][i, j], ref["rel"][i, j])
    top.close()
