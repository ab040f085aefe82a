"""CPU checks of the table digest's numpy restatement (tests/table_digest.py, what the
GPU tests in test_gpu_table_digest.py compare the device against) on values written
out in Python integers, and of dist.replica_parity on a gloo world of 2."""
import os

import numpy as np
import pytest

import table_digest as td

M64 = (1 << 64) - 1


def py_mix(x):
    """include/spe.h's mix, in Python integers."""
    x &= M64
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    x ^= x >> 31
    return x


def f64_bits(v):
    return int(np.float64(v).view(np.uint64))


def py_digest(rows, A, b):
    """Block b's four digests, term by term."""
    out = [0, 0, 0, 0]
    for s in range(64 * b, min(A, 64 * b + 64)):
        for t in range(A):
            km = py_mix(s * A + t + 1)
            bits = (f64_bits(rows["lat"][s, t]), f64_bits(rows["rel"][s, t]), int(rows["next"][s, t]) & 0xFFFFFFFF,
                    int(rows["hops"][s, t]) & 0xFFFF)
            for f in range(4):
                out[f] = (out[f] + py_mix(bits[f] + km * (2 * f + 1))) & M64
    return out


def test_mix_against_hand_computed_values():
    # the first three outputs of splitmix64 seeded with 0: mix(k * 0x9E3779B97F4A7C15), k = 1, 2, 3
    g = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    x = [(k * g) & M64 for k in (1, 2, 3)]
    assert [py_mix(v) for v in x] == want
    assert td.mix(np.array(x, np.uint64)).tolist() == want
    assert int(td.mix(np.uint64(0))[0]) == 0 == py_mix(0)
    # a bijection: distinct inputs, distinct outputs (here over a small range), wrapping arithmetic
    v = td.mix(np.arange(1 << 16, dtype=np.uint64))
    assert np.unique(v).size == 1 << 16
    assert int(td.mix(np.uint64(M64))[0]) == py_mix(M64)


def test_three_by_three_table_term_by_term():
    rows = {"lat": np.array([[-1.0, 2.5, 7.25], [2.5, -1.0, 1e-3], [7.25, 0.125, 3.0]]),
            "rel": np.array([[-1.0, 1.0, 0.5], [0.99, -1.0, 0.0], [0.75, 1.0, 1.0]]),
            "next": np.array([[-1, 1, 2], [0, -1, 70000], [1, 1, 2]], np.int32),
            "hops": np.array([[0, 1, 2], [1, 0, 65535], [2, 1, 2]], np.int32)}
    got = td.block_digests(rows, 3, 0, 1)
    assert got.shape == (1, 4) and got.dtype == np.uint64
    assert got[0].tolist() == py_digest(rows, 3, 0)
    # the unroutable next hop -1 enters as 0xFFFFFFFF, not sign-extended
    km = py_mix(0 * 3 + 0 + 1)
    assert py_mix(0xFFFFFFFF + km * 5) != py_mix(M64 + km * 5)
    only = {k: v[:1, :1] for k, v in rows.items()}
    assert int(td.block_digests(only, 1, 0, 1)[0, 2]) == py_mix(0xFFFFFFFF + km * 5)


def test_swapping_two_entries_of_a_row_changes_that_block():
    A = 130
    rows = td.seeded_rows(A, 1)
    base = td.block_digests(rows, A, 0, 3)
    assert base[2].tolist() == py_digest(rows, A, 2)             # the short last block, term by term
    for f, k in enumerate(td.FIELDS):
        sw = {n: np.array(v) for n, v in rows.items()}
        s, t1, t2 = 70, 3, 90
        assert sw[k][s, t1] != sw[k][s, t2]
        sw[k][s, t1], sw[k][s, t2] = rows[k][s, t2], rows[k][s, t1]
        got = td.block_digests(sw, A, 0, 3)
        changed = got != base
        assert changed[1, f] and changed.sum() == 1, (k, changed)   # the same values at other keys: another sum


def test_moving_a_row_to_another_block_changes_both_blocks():
    A = 130
    rows = td.seeded_rows(A, 2)
    base = td.block_digests(rows, A, 0, 3)
    mv = {n: np.array(v) for n, v in rows.items()}
    for n in mv:
        mv[n][[3, 70]] = rows[n][[70, 3]]
    got = td.block_digests(mv, A, 0, 3)
    assert (got[0] != base[0]).all() and (got[1] != base[1]).all() and (got[2] == base[2]).all()


def test_block_range_equals_the_same_blocks_of_the_whole():
    A = 200
    rows = td.seeded_rows(A, 3)
    whole = td.block_digests(rows, A, 0, 4)
    for b0, b1 in ((1, 3), (3, 4), (0, 1), (2, 4)):
        part = {k: v[64 * b0:min(A, 64 * b1)] for k, v in rows.items()}
        assert np.array_equal(td.block_digests(part, A, b0, b1), whole[b0:b1]), (b0, b1)


# ---- dist.replica_parity, one process per rank over gloo ----------------------------------------

def _parity_worker(rank, world, port, out_q):
    import torch.distributed as dist
    from shadow_amd import dist as sd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    A = 130                                                      # three blocks, split 2 + 1
    rows = td.seeded_rows(A, 4)
    dg = td.block_digests(rows, A, 0, 3)[:, :2]
    mask = np.array([True, True, False]) if rank == 0 else np.array([False, False, True])
    junk = np.full((3, 2), 0xDEADBEEF + rank, np.uint64)          # rows outside the mask are ignored
    built = np.where(mask[:, None], dg, junk)
    res = {"clean": sd.replica_parity(built, mask, dg, dist)}
    # rank 1's gathered copy of block 0 with one record changed
    gathered = dg.copy()
    if rank == 1:
        bad = {k: np.array(v) for k, v in rows.items()}
        bad["lat"][5, 7] = np.nextafter(bad["lat"][5, 7], np.inf)
        gathered = td.block_digests(bad, A, 0, 3)[:, :2]
        assert (gathered[0] != dg[0]).sum() == 1 and (gathered[1:] == dg[1:]).all()
    res["damaged"] = sd.replica_parity(built, mask, gathered, dist)
    # nobody claims block 1: counted, and its digests are not compared
    mask2 = np.array([True, False, False]) if rank == 0 else np.array([False, False, True])
    g2 = dg.copy()
    g2[1] += np.uint64(rank + 1)
    res["unbuilt"] = sd.replica_parity(np.where(mask2[:, None], dg, junk), mask2, g2, dist)
    # a block built by both ranks takes its reference from the lower one
    both = np.array([True, True, True]) if rank == 0 else np.array([False, False, True])
    b3 = np.where(both[:, None], dg, junk)
    if rank == 1:
        b3[2, 0] += np.uint64(1)                                  # rank 1's own build of block 2 differs ...
    g3 = dg.copy() if rank == 0 else np.where(np.arange(3)[:, None] == 2, b3, dg)   # ... and sits in its span
    res["overlap"] = sd.replica_parity(b3, both, g3, dist)
    out_q.put((rank, res))
    dist.destroy_process_group()


def test_replica_parity_gloo_world2():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_parity_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res[0] == res[1]                                       # identical on every rank
    r = res[0]
    assert r["clean"] == {"ranks": 2, "blocks": 3, "mismatching_blocks": 0, "first_bad": None, "unbuilt_blocks": 0}
    assert r["damaged"] == {"ranks": 2, "blocks": 3, "mismatching_blocks": 1, "first_bad": (1, 0), "unbuilt_blocks": 0}
    assert r["unbuilt"] == {"ranks": 2, "blocks": 3, "mismatching_blocks": 0, "first_bad": None, "unbuilt_blocks": 1}
    assert r["overlap"] == {"ranks": 2, "blocks": 3, "mismatching_blocks": 1, "first_bad": (1, 2), "unbuilt_blocks": 0}


def test_replica_parity_rejects_misshapen_arrays():
    from shadow_amd import dist as sd
    with pytest.raises(ValueError):
        sd.replica_parity(np.zeros((3, 2), np.uint64), np.ones(3, bool), np.zeros((2, 2), np.uint64), None)
