"""Measure spe_table_digest on one MI355X (MEASUREMENTS.md, "Table digests").

On the C3 table (bench.py's default workload and slot order: Barabasi-Albert
n = 50000, every vertex attached) it times, alternating in one process after a
warm-up call of each:
  * spe_table_digest over all blocks: 22 algorithmic bytes per (s, t) pair (the
    16-B {latency, reliability} record, the 4-B next hop, the 2-B hop count);
  * spe_table_compare of the table against a second build: the same fields of two
    tables, 44 bytes per pair -- the existing kernel that streams what the digest
    streams, hence the yardstick: the digest's bytes per second should not fall
    below the compare's, or the hashing binds.
Times are host clocks around the calls (each ends in a device synchronise and
includes its allocation and read-back: what a caller pays).  Then a
devices=[0, 0] build with verify_replicas: verify_seconds next to seconds and
gather_seconds.  One JSON object on stdout.

    python tools/measure_digest.py [--n 50000] [--reps 20] [--no-multi]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shadow_amd import graphs, spe  # noqa: E402

DIGEST_BYTES, COMPARE_BYTES, HBM_PEAK = 22, 44, 8.0e12


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def rate(pairs, nbytes, seconds):
    med = statistics.median(seconds)
    return {"median_s": med, "min_s": min(seconds), "max_s": max(seconds), "reps": len(seconds),
            "GBps_median": pairs * nbytes / med / 1e9, "GBps_best": pairs * nbytes / min(seconds) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000, help="vertices of the Barabasi-Albert graph (C3: 50000)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-multi", action="store_true", help="skip the devices=[0, 0] build")
    args = ap.parse_args()
    if spe.device_count() < 1:
        raise SystemExit("measure_digest: no GPU visible (nothing is measured without one)")
    top = graphs.gen_ba(args.n, 3, 3)
    g = spe.Graph(top)
    att = g.order_sources(np.arange(top.n, dtype=np.int32))
    A = int(att.shape[0])
    pairs = A * A
    out = {"graph": f"Barabasi-Albert n={args.n} m=3 seed=3", "n_attached": A, "blocks": (A + 63) // 64, "pairs": pairs}

    a = spe.PathTable(g, att)
    out["build_seconds"] = a.build()["seconds"]
    b = spe.PathTable(g, att)
    b.build()
    first = a.digest()                      # warm-up of each (code objects, first launches)
    rep = a.compare(b)
    out["compare_report"] = {k: rep[k] for k in ("pairs", "route_mismatch", "latency_differs", "reliability_differs")}
    out["digests_equal_between_builds"] = bool(np.array_equal(first, b.digest()))
    td, tc = [], []
    for _ in range(args.reps):              # alternating: both see the same machine
        td.append(timed(a.digest))
        tc.append(timed(lambda: a.compare(b)))
    out["digest_repeatable"] = bool(np.array_equal(first, a.digest()))
    out["digest"] = rate(pairs, DIGEST_BYTES, td)
    out["compare"] = rate(pairs, COMPARE_BYTES, tc)
    out["digest_over_compare_bytes_per_second"] = out["digest"]["GBps_median"] / out["compare"]["GBps_median"]
    out["digest_share_of_8TBps_peak"] = out["digest"]["GBps_median"] * 1e9 / HBM_PEAK
    a.close()
    b.close()

    if not args.no_multi:
        m = spe.PathTable(g, att, devices=[0, 0], verify_replicas=True)
        st = m.build()
        out["multi_devices_0_0"] = {k: st[k] for k in ("seconds", "gather_seconds", "build_wait_seconds", "verify_seconds",
                                                       "replica_mismatches", "shared_blocks", "local_blocks")}
        again = m.verify_replicas()
        out["multi_devices_0_0"]["verify_again"] = again
        # two replicas x 16 B per pair, both on the one device here
        out["multi_devices_0_0"]["verify_GBps"] = 2 * pairs * 16 / again["seconds"] / 1e9
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
