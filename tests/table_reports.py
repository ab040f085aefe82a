"""numpy reference of the table utilities' contracts in include/spe.h: the SB64
layout (spe_table_layout), spe_table_compare's report (spe_compare_report),
spe_table_check's report (spe_check_report) and the answers of spe_lookup_batch.

Written from the header's comments, not from the kernels, so that the GPU tests
in test_gpu_table_reports.py compare the device against an independent statement
of what it should count.  tests/test_table_reports.py checks this module on
hand-made tables whose counts are written out in the test.

Row-major tables are dicts of [rows, A] arrays: lat / rel float64, next int32,
hops int32 (0 .. 65535).  The device keeps hops as uint16; torch has no uint16,
so device buffers carry the int16 bit pattern: hops_to_i16 / hops_from_i16 are
the one place that converts.
"""
import numpy as np

WAVE = 64
FIELDS = ("lat", "rel", "next", "hops")


def nblocks(A):
    return (A + WAVE - 1) // WAVE


def hops_to_i16(h):
    """hops 0 .. 65535 -> the int16 bit pattern of the device's uint16."""
    h = np.asarray(h)
    assert ((h >= 0) & (h <= 0xFFFF)).all()
    return h.astype(np.uint16).view(np.int16)


def hops_from_i16(x):
    return np.ascontiguousarray(x, np.int16).view(np.uint16).astype(np.int32)


def sb64_offset(A, blk0, s, t):
    """Element (s, t) of a table owning blocks from blk0 on (spe_table_layout):
    ((s / 64 - blk0) * A + t) * 64 + s % 64.  Scalars or int64 arrays."""
    s = np.asarray(s, np.int64)
    t = np.asarray(t, np.int64)
    return ((s // WAVE - blk0) * A + t) * WAVE + s % WAVE


def owned_rows(A, blk0, blk1):
    """[first, one past the last) source slot of blocks [blk0, blk1)."""
    return blk0 * WAVE, min(A, blk1 * WAVE)


def padding_mask(A, blk0, blk1):
    """bool per SB64 element of the span: True in lanes with no source (s >= A)."""
    m = np.zeros((blk1 - blk0, A, WAVE), bool)
    if blk1 * WAVE > A and blk1 > blk0:
        m[nblocks(A) - 1 - blk0, :, A % WAVE:] = True
    return m.reshape(-1)


def pack_sb64(rows, A, blk0, blk1, pad):
    """Row-major owned rows [r1 - r0, A, ...] -> the SB64 span of blocks
    [blk0, blk1), [(blk1 - blk0) * A * 64, ...].  Padding lanes take `pad`: a
    scalar, or an array of the span's shape whose padding elements are used."""
    rows = np.asarray(rows)
    r0, r1 = owned_rows(A, blk0, blk1)
    assert rows.shape[:2] == (r1 - r0, A), (rows.shape, r0, r1, A)
    tail = rows.shape[2:]
    out = np.empty((blk1 - blk0, A, WAVE) + tail, rows.dtype)
    out[...] = np.asarray(pad, rows.dtype).reshape(out.shape) if np.ndim(pad) else pad
    for b in range(blk0, blk1):
        lo, hi = b * WAVE, min(A, (b + 1) * WAVE)
        out[b - blk0, :, :hi - lo] = np.swapaxes(rows[lo - r0:hi - r0], 0, 1)
    return out.reshape((-1,) + tail)


def unpack_sb64(span, A, blk0, blk1):
    """The SB64 span of blocks [blk0, blk1) -> row-major owned rows [r1 - r0, A, ...]."""
    span = np.asarray(span)
    r0, r1 = owned_rows(A, blk0, blk1)
    tail = span.shape[1:]
    v = span.reshape((blk1 - blk0, A, WAVE) + tail)
    rows = np.empty((r1 - r0, A) + tail, span.dtype)
    for b in range(blk0, blk1):
        lo, hi = b * WAVE, min(A, (b + 1) * WAVE)
        rows[lo - r0:hi - r0] = np.swapaxes(v[b - blk0, :, :hi - lo], 0, 1)
    return rows


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _pairs(mask, row0):
    s, t = np.nonzero(mask)
    return set(zip((s + row0).tolist(), t.tolist()))


def compare_report(a, b, tol, row0=0):
    """spe_compare_report of tables a and b (row-major dicts over the same owned
    rows, the first of which is slot row0), plus "bad": the set of (s, t) the
    device may report as first_bad (route mismatch or out of tolerance).

    An entry is routable when its latency is > -1 (topology_isRoutable).  Values
    are compared where both entries are routable: an unroutable entry has no
    latency to be within tolerance of and delivers no packet whose time could flip."""
    la, lb = np.asarray(a["lat"], np.float64), np.asarray(b["lat"], np.float64)
    ra, rb = np.asarray(a["rel"], np.float64), np.asarray(b["rel"], np.float64)
    oa, ob = la > -1.0, lb > -1.0
    route = (oa != ob) | (np.asarray(a["next"]) != np.asarray(b["next"])) | (np.asarray(a["hops"]) != np.asarray(b["hops"]))
    both = oa & ob
    with np.errstate(all="ignore"):
        dl = np.where(la == lb, 0.0, np.abs(la - lb) / np.abs(lb))
        dr = np.where(ra == rb, 0.0, np.abs(ra - rb) / np.abs(rb))
        out = both & ((np.where(la == lb, False, ~(np.abs(la - lb) <= tol * np.abs(lb)))) |
                      (np.where(ra == rb, False, ~(np.abs(ra - rb) <= tol * np.abs(rb)))))
        flips = both & (np.ceil(la * 1e6) != np.ceil(lb * 1e6))
    return {
        "pairs": int(la.size),
        "routable": int(ob.sum()),
        "route_mismatch": int(route.sum()),
        "latency_differs": int((both & (_bits(la) != _bits(lb))).sum()),
        "reliability_differs": int((both & (_bits(ra) != _bits(rb))).sum()),
        "beyond_tolerance": int(out.sum()),
        "delivery_flips": int(flips.sum()),
        "max_latency_rel_err": float(dl[both].max()) if both.any() else 0.0,
        "max_reliability_rel_err": float(dr[both].max()) if both.any() else 0.0,
        "bad": _pairs(route | out, row0),
    }


def check_report(top, attached, tab):
    """spe_check_report of the whole row-major table `tab` over the attached
    vertices of Topology `top`, every (s, t) with s != t, plus "bad": the set of
    (s, t) failing any rule.

    routable (latency > -1) entries only; one that fails bad_values takes no
    further check.  Adjacent: an edge s -> next exists (either direction on an
    undirected graph).  Hop rule where next is attached and is not t.  Symmetry
    (undirected graphs only) of (s, t) against whatever (t, s) holds, relative to
    (s, t)'s own values."""
    attached = np.asarray(attached, np.int64)
    A, n = attached.shape[0], int(top.n)
    lat, rel = np.asarray(tab["lat"], np.float64), np.asarray(tab["rel"], np.float64)
    nxt, hops = np.asarray(tab["next"], np.int64), np.asarray(tab["hops"], np.int64)
    assert lat.shape == (A, A)
    slot = np.full(n, -1, np.int64)
    slot[attached] = np.arange(A)
    src, dst = np.asarray(top.esrc, np.int64), np.asarray(top.edst, np.int64)
    edges = src * n + dst
    if not top.directed:
        edges = np.concatenate([edges, dst * n + src])
    edges = np.unique(edges)

    off = ~np.eye(A, dtype=bool)
    routable = off & (lat > -1.0)
    badv = routable & ~((lat > 0.0) & (rel > 0.0) & (rel <= 1.0) & (hops >= 1) & (nxt >= 0) & (nxt < n))
    good = routable & ~badv
    nx = np.where(good, nxt, 0)
    sv = attached[:, None]
    tv = attached[None, :]
    nna = good & ~np.isin(sv * n + nx, edges)
    xs = slot[nx]
    hopc = good & (xs >= 0) & (nx != tv)
    h2 = hops[np.where(hopc, xs, 0), np.arange(A)[None, :]]
    hopm = hopc & (hops != 1 + h2)
    symc = good if not top.directed else np.zeros_like(good)
    with np.errstate(all="ignore"):
        d = np.maximum(np.abs(lat - lat.T) / lat, np.abs(rel - rel.T) / rel)
    symm = symc & ~(d <= 1e-12)
    return {
        "pairs": int(off.sum()),
        "unroutable": int((off & ~routable).sum()),
        "bad_values": int(badv.sum()),
        "next_not_adjacent": int(nna.sum()),
        "hop_checked": int(hopc.sum()),
        "hop_mismatch": int(hopm.sum()),
        "sym_checked": int(symc.sum()),
        "sym_mismatch": int(symm.sum()),
        "max_sym_rel_err": float(d[symc].max()) if symc.any() else 0.0,
        "bad": _pairs(badv | nna | hopm | symm, 0),
    }


def lookup_answers(rows_lat, rows_rel, A, blk0, blk1, pairs):
    """spe_lookup_batch's answers for (q, 2) slot pairs against the owned rows
    (row-major, as owned_rows(A, blk0, blk1)): the entry when both slots are
    attached slots (0 <= s, t < A) and s's block is owned, else (-1, -1);
    ok = latency > -1."""
    p = np.asarray(pairs, np.int64)
    s, t = p[:, 0], p[:, 1]
    r0, r1 = owned_rows(A, blk0, blk1)
    valid = (s >= r0) & (s < r1) & (t >= 0) & (t < A)
    si, ti = np.where(valid, s - r0, 0), np.where(valid, t, 0)
    lat = np.where(valid, np.asarray(rows_lat)[si, ti], -1.0)
    rel = np.where(valid, np.asarray(rows_rel)[si, ti], -1.0)
    return lat, rel, (lat > -1.0).astype(np.uint8)
