"""The topology drop-in's SHADOW_SPE_EXACT_DELIVERY seal (shadow_amd/host/shd_topology_spe.c):
exact_sources = 0 with exact_delivery = 1, answering the packet delays of the
SHADOW_SPE_EXACT_SOURCES = 1 seal.  One case: shape b of tests/exact_delivery_cases.py
(derived rows, pendant sources and targets) on the 10-ns grid with one edge off it, written
as GraphML; the same 10^5 random pairs through topology_getPathInfoBatch on both seals."""
import re

import numpy as np
import pytest

import exact_delivery_cases as ec
from shadow_amd import graphs

pytestmark = [pytest.mark.gpu, pytest.mark.engine_fixed, pytest.mark.shared_trees]


def sealed(tmp_path, monkeypatch, top, ips, verts, name, env):
    from shadow_amd import topology as T
    for k in ("SHADOW_SPE_EXACT_DELIVERY", "SHADOW_SPE_EXACT_SOURCES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SHADOW_SPE_ENGINE", "1")   # the batch engine (the graph would fit the LDS engine)
    monkeypatch.setenv(env, "1")
    p = tmp_path / name
    graphs.write_graphml(top, str(p), ips=ips)
    t = T.Topology(str(p))
    t.capture_logs()
    addrs = []
    for i, v in enumerate(verts):
        a = T.ip(f"11.{i // 60000}.{(i // 250) % 240}.{i % 250 + 1}")
        t.attach(a, ip_hint=ips[v])
        addrs.append(a)
    assert t.seal() == 0
    T.lib().topology_set_log_level(t.h, 0)   # the seal's lines are what is read: no per-query lines into Python
    return t, np.array(addrs, np.uint32)


def test_shim_exact_delivery_seal_answers_the_exact_delays(tmp_path, monkeypatch):
    top, verts = ec.grid_case("b")
    ips = [f"10.{v // 250}.{v % 250}.{1 + v % 7}" for v in range(top.n)]
    q = np.random.default_rng(7).integers(0, len(verts), (100_000, 2))
    # both seals first (the environment is read at the seal), then the queries
    d, ad = sealed(tmp_path, monkeypatch, top, ips, verts, "delivery.graphml", "SHADOW_SPE_EXACT_DELIVERY")
    e, ae = sealed(tmp_path, monkeypatch, top, ips, verts, "exact.graphml", "SHADOW_SPE_EXACT_SOURCES")
    line = [t for _, t in d.logs if "exact delivery" in t]
    assert len(line) == 1, d.logs
    m = re.search(r"delivery_flagged (\d+) delivery_changed (\d+) delivery_fallback (\d+) delivery_seconds ([0-9.]+)",
                  line[0])
    assert m, line
    # (on the grid every offset entry is flagged: with the default delivery_refold_max the blocks
    # holding offset rows go over their cap and are rebuilt, delivery_fallback 2)
    assert int(m.group(1)) > 0 and int(m.group(3)) in (0, 2) and float(m.group(4)) > 0, line
    assert not [t for _, t in e.logs if "exact delivery" in t]
    okd, latd, _ = d.path_info_batch(ad[q[:, 0]], ad[q[:, 1]])
    oke, late, _ = e.path_info_batch(ae[q[:, 0]], ae[q[:, 1]])
    d.close()
    e.close()
    np.testing.assert_array_equal(okd, oke)
    np.testing.assert_array_equal(np.ceil(latd * 1e6), np.ceil(late * 1e6))
