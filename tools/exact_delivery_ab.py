#!/usr/bin/env python3
"""A/B of spe_table_opts.exact_delivery on the bench's C3 and C4 tables.

Per config, in ONE process, on the bench's graph and slot order (bench.workload,
spe_order_sources), alternating per round
    the default build  |  exact_delivery = 1  |  exact_sources = 1
into one shared set of caller buffers: `--builds` timed whole-table builds each after
`--warmup` warm-ups.  Then, on tables of their own (C4 in quarters of the source blocks, as
bench.default_vs_exact: two whole C4 tables do not fit one device),
spe_table_compare(delivery, exact) and spe_table_compare(default, exact).  One JSON object
per config on stdout (and into --out):
    median and min-max build seconds of the three, the delivery_* stats, both comparisons,
    and (--resources) the DELIVERY = false row kernels' register counts.

--sweep: the default of delivery_refold_max.  On C3 a fraction of the edge latencies is
snapped to the ns grid (an entry is at an ns boundary when every edge of its path is, so the
flagged share of the offset entries grows steeply with the fraction); per fraction the
exact_delivery build with delivery_refold_max = 1 (every flagged entry re-folded,
no block rebuilt) is timed against the exact_sources build of the same table.  The flagged
share of a block's 64 * A entries at which the two cost the same is interpolated; the library
ships half of it (the walk length varies with the graph).

--kernel-resources OUT: no GPU; compiles the library's kernels with the compiler's resource
remarks and writes the row kernels' VGPRs / spills / waves per SIMD as JSON (--source-root:
another checkout, e.g. the parent commit's, to compare with).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATS = ("delivery_flagged", "delivery_changed", "delivery_fallback", "delivery_seconds", "relaxed_lanes",
         "derived_sources", "fallback_blocks")
ROW_KERNELS = ("k_rows_lm", "k_rows_shared_lds", "k_rows_sssp", "k_refold_delivery")


def kernel_resources(source_root, out):
    from shadow_amd import build_native as bn
    src = os.path.join(source_root, "shadow_amd", "csrc", "spe.hip")
    cmd = [bn.HIPCC, *bn.HIP_FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, src]
    txt = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    res, cur = {}, None
    for line in txt.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"^void \(anonymous namespace\)::", "", name).split("(")[0]
            cur = name if name.startswith(ROW_KERNELS) else None
            if cur:
                res[cur] = {}
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][A-Za-z \[\]/]+): (\d+)", line)
        if cur and m and m.group(1).strip() in ("VGPRs", "AGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                                                "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"):
            res[cur][m.group(1).strip()] = int(m.group(2))
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def build_modes():
    return {"default": dict(exact_sources=False), "delivery": dict(exact_sources=False, exact_delivery=True),
            "exact": dict(exact_sources=True)}


def timed_builds(spe, torch, g, order, modes, builds, warmup):
    """Alternating whole-table builds of every mode into one shared set of caller buffers."""
    A = len(order)
    nblk = (A + 63) // 64
    n = nblk * A * 64
    bufs = [torch.empty((n, 2), dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
            torch.empty(n, dtype=torch.int16, device="cuda")]
    tabs = {k: spe.PathTable(g, order, ext=[b.data_ptr() for b in bufs], **kw) for k, kw in modes.items()}
    secs = {k: [] for k in modes}
    last = {}
    for r in range(warmup + builds):
        for k, t in tabs.items():
            t0 = time.perf_counter()
            st = t.build()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r >= warmup:
                secs[k].append(dt)
            last[k] = st
    for t in tabs.values():
        t.close()
    del bufs
    torch.cuda.empty_cache()
    return secs, last


def compares(spe, g, order, parts):
    import numpy as np
    nblk = (len(order) + 63) // 64
    cuts = np.linspace(0, nblk, parts + 1).astype(int)
    tot = {"delivery_vs_exact": {}, "default_vs_exact": {}}
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        tabs = {k: spe.PathTable(g, order, blocks=(int(b0), int(b1)), **kw) for k, kw in build_modes().items()}
        for t in tabs.values():
            t.build()
        for name, a in (("delivery_vs_exact", "delivery"), ("default_vs_exact", "default")):
            r = tabs[a].compare(tabs["exact"], 1e-9)
            for k, v in r.items():
                if k.startswith("max_"):
                    tot[name][k] = max(tot[name].get(k, 0.0), v)
                elif not k.startswith("first_"):
                    tot[name][k] = tot[name].get(k, 0) + v
        for t in tabs.values():
            t.close()
    tot["parts"] = parts
    return tot


def run_config(config, args, resources):
    import torch
    import bench
    from shadow_amd import spe
    top, att, desc = bench.workload(config)
    g = spe.Graph(top)
    order = g.order_sources(att)
    secs, last = timed_builds(spe, torch, g, order, build_modes(), args.builds, args.warmup)
    out = {"config": config, "workload": desc, "attached": len(order), "builds": args.builds, "warmup": args.warmup,
           "build_seconds": {k: spread(v) for k, v in secs.items()},
           "delivery_stats": {k: last["delivery"][k] for k in STATS},
           "default_stats": {k: last["default"][k] for k in STATS},
           "exact_stats": {k: last["exact"][k] for k in STATS}}
    d, x, e = (out["build_seconds"][k]["median"] for k in ("default", "delivery", "exact"))
    out["delivery_over_default"] = x / d
    out["delivery_over_exact"] = x / e
    if not args.no_compare:
        out["compare"] = compares(spe, g, order, 4 if config == "c4" else 1)
    if resources:
        out["kernel_resources"] = resources
    g.close()
    return out


def run_sweep(args):
    """C3 with a fraction of the edge latencies snapped to the ns grid (see the module text)."""
    import numpy as np
    import torch
    import bench
    from shadow_amd import spe
    rows = []
    for frac in args.sweep_fractions:
        top, att, _ = bench.workload("c3")
        rng = np.random.default_rng(17)
        snap = (rng.random(top.m) < frac) & (top.esrc != top.edst)
        top.elat = np.where(snap, np.round(top.elat * 1e6) / 1e6, top.elat)
        g = spe.Graph(top)
        order = g.order_sources(att)
        modes = {"delivery": dict(exact_sources=False, exact_delivery=True, delivery_refold_max=1.0),
                 "default": dict(exact_sources=False), "exact": dict(exact_sources=True)}
        secs, last = timed_builds(spe, torch, g, order, modes, args.sweep_builds, 1)
        A = len(order)
        st = last["delivery"]
        rows.append({"edge_fraction": frac, "snapped_edges": int(snap.sum()),
                     "flagged_share": st["delivery_flagged"] / (float(A) * A),
                     "delivery_flagged": st["delivery_flagged"], "delivery_changed": st["delivery_changed"],
                     "delivery_seconds": st["delivery_seconds"], "fallback_blocks": st["fallback_blocks"],
                     "seconds": {k: spread(v) for k, v in secs.items()}})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        g.close()
    # the share at which default + re-fold costs what the exact build costs (linear between samples)
    even = None
    for a, b in zip(rows[:-1], rows[1:]):
        da = a["seconds"]["delivery"]["median"] - a["seconds"]["exact"]["median"]
        db = b["seconds"]["delivery"]["median"] - b["seconds"]["exact"]["median"]
        if da <= 0.0 < db:
            even = a["flagged_share"] + (b["flagged_share"] - a["flagged_share"]) * (-da) / (db - da)
            break
    return {"config": "c3-sweep", "rows": rows, "break_even_flagged_share": even,
            "default_delivery_refold_max": None if even is None else even / 2}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-compare", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-fractions", type=lambda s: [float(x) for x in s.split(",")],
                    default=[0.0, 0.3, 0.5, 0.7, 0.85, 0.95])
    ap.add_argument("--sweep-builds", type=int, default=3)
    ap.add_argument("--resources", default=None, help="JSON written by --kernel-resources, merged into every object")
    ap.add_argument("--kernel-resources", default=None, metavar="OUT")
    ap.add_argument("--source-root", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_resources:
        kernel_resources(args.source_root, args.kernel_resources)
        return
    resources = json.load(open(args.resources)) if args.resources else None
    objs = []
    for c in [c for c in args.configs.split(",") if c]:
        objs.append(run_config(c, args, resources))
        print(json.dumps(objs[-1]), flush=True)
    if args.sweep:
        objs.append(run_sweep(args))
        print(json.dumps(objs[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(objs, f, indent=1)


if __name__ == "__main__":
    main()
