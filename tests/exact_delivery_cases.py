"""Shapes and weightings of the exact_delivery tests (tests/test_gpu_exact_delivery*.py).

Three shapes, each small, none with an attached count that is a multiple of 64:
  a  gen_ba(3000, 3), all attached: contracted, derived rows (k_stage_lanes + k_rows_lm);
  b  a + 400 pendant vertices: derived rows with pendant sources and pendant targets;
  c  gen_tiered(1500, 6000, 3000): stubs on a plain core (k_rows_shared_lds).
Two weightings: `real` as generated; `grid` on the 10-ns grid, k * 1e-5 ms with k in
[1e5, 6e6) -- every path sum is at an ns boundary, yet fine enough that exact ties are rare
and most blocks keep their shared / derived rows.
"""
import numpy as np

from shadow_amd import graphs

# seed of the graph and of its grid weights, per shape (fallback_blocks of the default build
# with the grid weighting: see tests/test_gpu_exact_delivery.py)
SEEDS = {"a": (31, 131), "b": (43, 143), "c": (35, 135)}
OFF_GRID_MS = 5000.00000033   # not at an ns boundary, and too long to lie on any shortest path


def with_pendants(top, k, seed):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, top.n, k)
    n2 = top.n + k
    return graphs.Topology(n=n2, esrc=np.concatenate([top.esrc, np.arange(top.n, n2)]).astype(np.int32),
                           edst=np.concatenate([top.edst, anc]).astype(np.int32),
                           elat=np.concatenate([top.elat, rng.uniform(0.5, 10.0, k)]),
                           eloss=np.concatenate([top.eloss, rng.uniform(0, 0.01, k)]),
                           vloss=np.zeros(n2), directed=False, prefer_direct=False)


def shape(name, seed=None):
    """(topology, attached vertices) of shape a / b / c."""
    seed = SEEDS[name][0] if seed is None else seed
    if name == "a":
        top = graphs.gen_ba(3000, 3, seed)
        return top, np.arange(top.n, dtype=np.int32)
    if name == "b":
        top = with_pendants(graphs.gen_ba(3000, 3, seed), 400, seed + 1)
        return top, np.arange(top.n, dtype=np.int32)
    if name == "c":
        top = graphs.gen_tiered(n_core=1500, n_stub=6000, n_attached=3000, seed=seed)
        return top, graphs.tiered_attached(top, 1500, 3000)
    raise KeyError(name)


def on_grid(top, seed, off_grid_edge=True):
    """Every edge latency on the 10-ns grid.  off_grid_edge: one edge is moved off the grid,
    so that spe_table_create does not predict the ns-grid case, and made longer than any
    path around it, so that it lies on no shortest path and every entry's path sum still is
    at an ns boundary: the first edge between two vertices of degree >= 3 (an edge into a
    vertex of degree 1 would lie on every path of that vertex)."""
    rng = np.random.default_rng(seed)
    top.elat = rng.integers(100_000, 6_000_000, top.elat.shape[0]) * 1e-5
    if off_grid_edge:
        plain = top.esrc != top.edst
        deg = np.bincount(np.concatenate([top.esrc[plain], top.edst[plain]]), minlength=top.n)
        e = int(np.flatnonzero(plain & (deg[top.esrc] >= 3) & (deg[top.edst] >= 3))[0])
        top.elat[e] = OFF_GRID_MS
    return top


def grid_case(name, off_grid_edge=True, seeds=None):
    gseed, wseed = SEEDS[name] if seeds is None else seeds
    top, A = shape(name, gseed)
    return on_grid(top, wseed, off_grid_edge), A
