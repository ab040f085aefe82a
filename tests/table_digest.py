"""numpy restatement of the per-block table digest of include/spe.h
(spe_block_digest, spe_table_digest), from row-major rows.

Written from the header's definition, not from the kernel:

    mix(x):  x ^= x >> 30;  x *= 0xbf58476d1ce4e5b9;
             x ^= x >> 27;  x *= 0x94d049bb133111eb;
             x ^= x >> 31                                  (uint64, wrapping)
    key(s, t)     = s * A + t                              (global slots)
    km(s, t)      = mix(key + 1)
    term(f, s, t) = mix(bits_f(s, t) + km * (2 f + 1))
    digest[b][f]  = sum of term(f, s, t), s in [64 b, min(64 b + 64, A)), t in [0, A)

fields f: 0 latency and 1 reliability (the f64 bit patterns), 2 next hop (int32 as
uint32, zero-extended), 3 hop count (uint16, zero-extended).  Only real rows enter:
a row-major table has no padding lanes.  tests/test_table_digest.py checks this
module against sums written out in Python integers.  seeded_rows makes the tables
both test files digest.
"""
import numpy as np

WAVE = 64
M1 = np.uint64(0xbf58476d1ce4e5b9)
M2 = np.uint64(0x94d049bb133111eb)
FIELDS = ("lat", "rel", "next", "hops")


def seeded_rows(A, seed, r0=0, r1=None):
    """Rows [r0, r1) of a seeded table: routable and unroutable entries, next hops of
    both signs, hop counts past 32768."""
    r1 = A if r1 is None else r1
    rng = np.random.default_rng(seed)
    rows = {"lat": rng.uniform(0.5, 900.0, (A, A)), "rel": rng.uniform(0.0, 1.0, (A, A)),
            "next": rng.integers(0, 10**6, (A, A)).astype(np.int32), "hops": rng.integers(1, 65536, (A, A)).astype(np.int32)}
    dead = rng.random((A, A)) < 0.05
    for k, v in (("lat", -1.0), ("rel", -1.0), ("next", -1), ("hops", 0)):
        rows[k][dead] = v
    return {k: v[r0:r1] for k, v in rows.items()}


def mix(x):
    """The splitmix64 finaliser on a uint64 array (or scalar), wrapping."""
    x = np.array(x, np.uint64, ndmin=1)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= M1
        x ^= x >> np.uint64(27)
        x *= M2
        x ^= x >> np.uint64(31)
    return x


def field_bits(rows):
    """The four fields' bits as uint64 arrays [rows, A], in digest order."""
    lat = np.ascontiguousarray(rows["lat"], np.float64).view(np.uint64)
    rel = np.ascontiguousarray(rows["rel"], np.float64).view(np.uint64)
    nxt = np.ascontiguousarray(rows["next"], np.int32).view(np.uint32).astype(np.uint64)
    hops = np.asarray(rows["hops"])
    assert ((hops >= 0) & (hops <= 0xFFFF)).all()
    return lat, rel, nxt, hops.astype(np.uint64)


def block_digests(rows, A, b0, b1):
    """uint64 [b1 - b0, 4]: the digests of blocks [b0, b1) from the row-major
    lat / rel / next / hops of exactly those blocks' source rows, i.e. slots
    [64 b0, min(A, 64 b1)) x [0, A)."""
    r0, r1 = b0 * WAVE, min(A, b1 * WAVE)
    bits = field_bits(rows)
    assert bits[0].shape == (r1 - r0, A), (bits[0].shape, r0, r1, A)
    out = np.zeros((b1 - b0, 4), np.uint64)
    t = np.arange(A, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for b in range(b0, b1):
            lo, hi = b * WAVE, min(A, (b + 1) * WAVE)
            s = np.arange(lo, hi, dtype=np.uint64)[:, None]
            km = mix((s * np.uint64(A) + t[None, :] + np.uint64(1)).ravel())
            for f in range(4):
                x = bits[f][lo - r0:hi - r0].ravel() + km * np.uint64(2 * f + 1)
                out[b - b0, f] = np.add.reduce(mix(x), dtype=np.uint64)
    return out
