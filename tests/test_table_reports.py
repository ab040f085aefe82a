"""The numpy reference of the table reports (tests/table_reports.py) on hand-made
tables whose expected counts are written out here, so that
test_gpu_table_reports.py does not compare two unverified things."""
import numpy as np
import pytest

import table_reports as tr
from shadow_amd.graphs import Topology


# ---- SB64 pack / unpack ----------------------------------------------------------------

def test_sb64_offset_by_hand():
    # A = 3: one block, element (s, t) at t * 64 + s
    assert tr.sb64_offset(3, 0, 0, 0) == 0
    assert tr.sb64_offset(3, 0, 2, 1) == 66
    # A = 70: block 1 starts after 70 * 64 elements
    assert tr.sb64_offset(70, 0, 63, 69) == 69 * 64 + 63
    assert tr.sb64_offset(70, 0, 64, 0) == 70 * 64
    assert tr.sb64_offset(70, 0, 69, 69) == (70 + 69) * 64 + 5
    # a table owning blocks from 1 on: block-relative
    assert tr.sb64_offset(70, 1, 64, 0) == 0
    assert tr.sb64_offset(70, 1, 69, 2) == 2 * 64 + 5
    assert tr.sb64_offset(300, 3, 256, 7) == (300 + 7) * 64
    np.testing.assert_array_equal(tr.sb64_offset(70, 0, np.array([1, 65]), np.array([2, 3])), [129, (70 + 3) * 64 + 1])


def test_pack_a3_by_hand():
    rows = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.int32)
    span = tr.pack_sb64(rows, 3, 0, 1, -7)
    assert span.shape == (3 * 64,)
    for t in range(3):
        assert span[t * 64:t * 64 + 3].tolist() == rows[:, t].tolist()   # 64 sources interleaved per target
        assert (span[t * 64 + 3:(t + 1) * 64] == -7).all()               # 61 padding lanes
    pm = tr.padding_mask(3, 0, 1)
    assert pm.sum() == 3 * 61 and (span[pm] == -7).all() and (span[~pm] != -7).all()
    np.testing.assert_array_equal(tr.unpack_sb64(span, 3, 0, 1), rows)


@pytest.mark.parametrize("blocks", [(0, 2), (0, 1), (1, 2)])
def test_pack_unpack_a70(blocks):
    A = 70
    b0, b1 = blocks
    r0, r1 = tr.owned_rows(A, b0, b1)
    assert (r0, r1) == {(0, 2): (0, 70), (0, 1): (0, 64), (1, 2): (64, 70)}[blocks]
    full = np.arange(A * A, dtype=np.float64).reshape(A, A) + 0.25
    garbage = -np.arange((b1 - b0) * A * 64, dtype=np.float64) - 1.0   # all negative: told apart from the rows
    span = tr.pack_sb64(full[r0:r1], A, b0, b1, garbage)
    pm = tr.padding_mask(A, b0, b1)
    assert pm.sum() == (58 * A if b1 == 2 else 0)
    assert (span[pm] < 0).all() and (span[~pm] > 0).all()
    np.testing.assert_array_equal(span[pm], garbage[pm])
    for s, t in ((r0, 0), (r1 - 1, A - 1), (r0 + 3, 17)):
        assert span[tr.sb64_offset(A, b0, s, t)] == full[s, t]
    np.testing.assert_array_equal(tr.unpack_sb64(span, A, b0, b1), full[r0:r1])
    # records with a trailing dimension ({latency, reliability})
    rec = np.stack([full[r0:r1], -full[r0:r1]], -1)
    sp2 = tr.pack_sb64(rec, A, b0, b1, np.nan)
    assert sp2.shape == ((b1 - b0) * A * 64, 2) and np.isnan(sp2[pm]).all()
    np.testing.assert_array_equal(tr.unpack_sb64(sp2, A, b0, b1), rec)


def test_hops_uint16_bit_pattern():
    h = np.array([0, 1, 32767, 32768, 40000, 65535], np.int32)
    i16 = tr.hops_to_i16(h)
    assert i16.dtype == np.int16 and i16.tolist() == [0, 1, 32767, -32768, 40000 - 65536, -1]
    np.testing.assert_array_equal(tr.hops_from_i16(i16), h)
    rows = np.full((3, 3), 40000, np.int32)
    span = tr.pack_sb64(tr.hops_to_i16(rows), 3, 0, 1, -1)
    np.testing.assert_array_equal(tr.hops_from_i16(tr.unpack_sb64(span, 3, 0, 1)), rows)


# ---- compare_report ----------------------------------------------------------------------

def _table(A, rows=None):
    rows = A if rows is None else rows
    s, t = np.meshgrid(np.arange(rows), np.arange(A), indexing="ij")
    return {"lat": 1.0 + s + t / 128.0, "rel": np.full((rows, A), 0.75), "next": (t % 5).astype(np.int32),
            "hops": (1 + (s + t) % 3).astype(np.int32)}


def _copy(tab):
    return {k: v.copy() for k, v in tab.items()}


ZERO = {"route_mismatch": 0, "latency_differs": 0, "reliability_differs": 0, "beyond_tolerance": 0,
        "delivery_flips": 0, "max_latency_rel_err": 0.0, "max_reliability_rel_err": 0.0, "bad": set()}


def test_compare_identical():
    b = _table(3)
    r = tr.compare_report(_copy(b), b, 1e-12)
    assert r == dict(ZERO, pairs=9, routable=9)


def test_compare_one_of_each_kind_a3():
    """Nine entries, six of them different in one way each."""
    b = _table(3)
    b["lat"][2, 2] = 0.5
    b["lat"][0, 1] = 2.0
    b["lat"][0, 0] = 1.0000005    # x 1e6 lies mid-way between two integers: one ulp moves no ceil()
    a = _copy(b)
    a["lat"][0, 0] = np.nextafter(b["lat"][0, 0], 9.0)     # +1 ulp: differs, within 1e-12, no flip
    a["lat"][0, 1] = b["lat"][0, 1] * (1 + 1e-9)           # beyond tolerance, and ceil(lat * 1e6) moves
    a["rel"][0, 2] = b["rel"][0, 2] * (1 - 1e-9)           # beyond tolerance in reliability
    a["next"][1, 0] = 4                                    # route
    a["hops"][1, 1] = 40000                                # route
    for k, v in (("lat", -1.0), ("rel", -1.0), ("next", -1), ("hops", 0)):
        a[k][1, 2] = v                                     # unroutable in a only
    a["lat"][2, 2] = np.nextafter(0.5, 1.0)                # delivery flip alone
    assert np.ceil(0.5 * 1e6) == 500000 and np.ceil(np.nextafter(0.5, 1.0) * 1e6) == 500001
    lat01 = b["lat"][0, 1]
    assert np.ceil(lat01 * 1e6) != np.ceil(lat01 * (1 + 1e-9) * 1e6)
    r = tr.compare_report(a, b, 1e-12)
    assert r["pairs"] == 9 and r["routable"] == 9
    assert r["route_mismatch"] == 3
    assert r["latency_differs"] == 3          # (0,0), (0,1), (2,2); (1,2) is not routable in both
    assert r["reliability_differs"] == 1
    assert r["beyond_tolerance"] == 2
    assert r["delivery_flips"] == 2
    assert r["max_latency_rel_err"] == abs(a["lat"][0, 1] - lat01) / lat01 and 0.9e-9 < r["max_latency_rel_err"] < 1.1e-9
    assert r["max_reliability_rel_err"] == abs(a["rel"][0, 2] - 0.75) / 0.75
    assert r["bad"] == {(0, 1), (0, 2), (1, 0), (1, 1), (1, 2)}
    # the other way round: routable counts table b
    r = tr.compare_report(b, a, 1e-12)
    assert r["routable"] == 8 and r["route_mismatch"] == 3 and r["latency_differs"] == 3
    # a looser tolerance takes the 1e-9 entries back in
    r = tr.compare_report(a, b, 1e-8)
    assert r["beyond_tolerance"] == 0 and r["bad"] == {(1, 0), (1, 1), (1, 2)}


def test_compare_error_is_relative_to_b():
    a, b = _table(3), _table(3)
    a["lat"][1, 2], b["lat"][1, 2] = 1.0, 2.0
    assert tr.compare_report(a, b, 1e-12)["max_latency_rel_err"] == 0.5
    assert tr.compare_report(b, a, 1e-12)["max_latency_rel_err"] == 1.0
    a, b = _table(3), _table(3)
    a["rel"][0, 1], b["rel"][0, 1] = 0.25, 1.0
    assert tr.compare_report(a, b, 1e-12)["max_reliability_rel_err"] == 0.75
    assert tr.compare_report(b, a, 1e-12)["max_reliability_rel_err"] == 3.0


def test_compare_a70_block_boundary_and_row_offset():
    b = _table(70)
    a = _copy(b)
    a["hops"][63, 69] += 1
    a["next"][64, 0] = 3 if b["next"][64, 0] != 3 else 2
    a["lat"][69, 69] *= 1 + 1e-9
    r = tr.compare_report(a, b, 1e-12)
    assert r["pairs"] == 4900 and r["routable"] == 4900
    assert r["route_mismatch"] == 2 and r["beyond_tolerance"] == 1 and r["latency_differs"] == 1
    assert r["bad"] == {(63, 69), (64, 0), (69, 69)}
    # the rows of block 1 alone: the set names absolute slots
    r = tr.compare_report({k: v[64:] for k, v in a.items()}, {k: v[64:] for k, v in b.items()}, 1e-12, row0=64)
    assert r["pairs"] == 6 * 70 and r["route_mismatch"] == 1 and r["bad"] == {(64, 0), (69, 69)}
    # hops of 40000 in both tables is no difference
    a, b = _table(70), _table(70)
    a["hops"][5, 5] = b["hops"][5, 5] = 40000
    assert tr.compare_report(a, b, 1e-12) == dict(ZERO, pairs=4900, routable=4900)


# ---- check_report ------------------------------------------------------------------------

def _path_graph(directed=False):
    """0 - 1 - 2 - 3 with latencies 1, 2, 4 (sums exact), no loss."""
    return Topology(n=4, esrc=np.array([0, 1, 2], np.int32), edst=np.array([1, 2, 3], np.int32),
                    elat=np.array([1.0, 2.0, 4.0]), eloss=np.zeros(3), vloss=np.zeros(4), directed=directed)


def _path_table(att=(0, 1, 2, 3)):
    pos = np.array([0.0, 1.0, 3.0, 7.0])
    att = np.asarray(att)
    s, t = np.meshgrid(att, att, indexing="ij")
    tab = {"lat": np.abs(pos[s] - pos[t]), "rel": np.ones(s.shape), "next": (s + np.sign(t - s)).astype(np.int32),
           "hops": np.abs(s - t).astype(np.int32)}
    tab["lat"][s == t] = 123.0   # the diagonal is not checked: anything goes
    tab["next"][s == t] = 99
    return tab


CLEAN = {"pairs": 12, "unroutable": 0, "bad_values": 0, "next_not_adjacent": 0, "hop_checked": 6, "hop_mismatch": 0,
         "sym_checked": 12, "sym_mismatch": 0, "max_sym_rel_err": 0.0, "bad": set()}


def _check(tab, top=None, att=(0, 1, 2, 3)):
    return tr.check_report(top or _path_graph(), np.asarray(att, np.int32), tab)


def test_check_clean_path_graph():
    # hop rule applies where the next hop is not the target: |s - t| >= 2, six ordered pairs
    assert _check(_path_table()) == CLEAN


def test_check_directed_graph_has_no_symmetry_check():
    top = _path_graph(directed=True)
    tab = _path_table()
    r = _check(tab, top)
    # edges only go up: every entry towards a lower vertex has a next hop with no edge s -> next
    assert r == dict(CLEAN, sym_checked=0, next_not_adjacent=6, bad={(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)})


@pytest.mark.parametrize("field,value", [("lat", 0.0), ("rel", 1.5), ("rel", 0.0), ("hops", 0), ("next", 4), ("next", -1)])
def test_check_bad_values(field, value):
    tab = _path_table()
    tab[field][0, 2] = value   # entry (0, 2): next 1, hops 2; hop rule and symmetry would apply
    r = _check(tab)
    exp = dict(CLEAN, bad_values=1, hop_checked=5, sym_checked=11, bad={(0, 2)})
    if field in ("lat", "rel"):   # (2, 0) still compares itself with (0, 2)
        exp.update(sym_mismatch=1, max_sym_rel_err={0.0: 1.0, 1.5: 0.5}[value], bad={(0, 2), (2, 0)})
    if field == "hops":           # (0, 3)'s hop rule reads hops(1, 3), nobody reads hops(0, 2)
        pass
    assert r == exp


def test_check_next_not_adjacent():
    tab = _path_table()
    tab["next"][0, 3] = 3      # the target itself, not a neighbour of 0: no hop check for this entry
    assert _check(tab) == dict(CLEAN, next_not_adjacent=1, hop_checked=5, bad={(0, 3)})
    tab["next"][0, 3] = 2      # not a neighbour either; 3 hops != 1 + hops(2, 3) = 2
    assert _check(tab) == dict(CLEAN, next_not_adjacent=1, hop_mismatch=1, bad={(0, 3)})


def test_check_hop_rule_counts_the_entry_and_its_readers():
    tab = _path_table()
    tab["hops"][1, 3] = 3      # (1, 3): 3 != 1 + hops(2, 3) = 2; (0, 3) goes through 1: 3 != 1 + 3
    assert _check(tab) == dict(CLEAN, hop_mismatch=2, bad={(1, 3), (0, 3)})
    tab = _path_table()
    tab["hops"][2, 3] = 2      # next is the target: no check of its own; read by (1, 3) only
    assert _check(tab) == dict(CLEAN, hop_mismatch=1, bad={(1, 3)})


def test_check_symmetry():
    tab = _path_table()
    tab["lat"][0, 2] = 3.0 * (1 + 1e-9)
    r = _check(tab)
    d = tab["lat"][0, 2] - 3.0
    assert r == dict(CLEAN, sym_mismatch=2, max_sym_rel_err=d / 3.0, bad={(0, 2), (2, 0)})
    assert d / 3.0 > d / tab["lat"][0, 2]    # relative to each entry's own value: the larger of the two
    tab = _path_table()
    tab["rel"][3, 1] = np.nextafter(1.0, 0.0)   # 1.1e-16: within 1e-12
    r = _check(tab)
    assert r == dict(CLEAN, max_sym_rel_err=(1.0 - tab["rel"][3, 1]) / tab["rel"][3, 1])


def test_check_unroutable_and_partial_attachment():
    tab = _path_table()
    for k, v in (("lat", -1.0), ("rel", -1.0), ("next", -1), ("hops", 0)):
        tab[k][0, 3] = v
    # (3, 0) compares its (7.0, 1.0) with (-1, -1): max(|7 + 1| / 7, |1 + 1| / 1)
    assert _check(tab) == dict(CLEAN, unroutable=1, hop_checked=5, sym_checked=11, sym_mismatch=1,
                               max_sym_rel_err=2.0, bad={(3, 0)})
    # vertices 0, 1, 3 attached: a next hop of 2 is no slot, so only (0, 3) via 1 and (3, 0)... via 2: one check
    att = (0, 1, 3)
    r = _check(_path_table(att), att=att)
    assert r == dict(CLEAN, pairs=6, hop_checked=1, sym_checked=6)


def test_lookup_answers():
    A = 70
    lat = np.arange(A * A, dtype=np.float64).reshape(A, A)
    lat[3, 4] = -1.0
    pairs = [(0, 0), (3, 4), (69, 69), (70, 0), (127, 0), (0, 70), (-1, 0), (0, -1), (64, 1), (2**31 - 1, 2**31 - 1)]
    L, R, ok = tr.lookup_answers(lat, -lat - 2, A, 0, 2, pairs)
    assert L.tolist() == [0.0, -1.0, 4899.0, -1.0, -1.0, -1.0, -1.0, -1.0, 64 * 70 + 1.0, -1.0]
    assert ok.tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 1, 0]
    assert R[0] == -2.0 and R[3] == -1.0
    L, R, ok = tr.lookup_answers(lat[64:], lat[64:], A, 1, 2, pairs)   # block 1 only
    assert L.tolist() == [-1.0, -1.0, 4899.0, -1.0, -1.0, -1.0, -1.0, -1.0, 64 * 70 + 1.0, -1.0]
