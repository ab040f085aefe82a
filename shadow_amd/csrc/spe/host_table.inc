// host_table.inc -- part of spe.hip (one translation unit).
// Host side: graph queries, source order, table creation and layout.

extern "C" {

int spe_graph_set_edge_aux(spe_graph* g, const double* edge_aux) {
    if (!g || (!edge_aux && g->hg.m > 0)) return fail(SPE_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(g->device));
    const spe::HostGraph& h = g->hg;
    for (int64_t e = 0; e < h.m; ++e)
        if (!std::isfinite(edge_aux[e])) return fail(SPE_EINVAL, "edge " + std::to_string(e) + " aux value is not finite");
    g->aux_edge.assign(edge_aux, edge_aux + h.m);
    std::vector<double> ia(h.ieid.size()), fa(h.fieid.size());
    for (size_t k = 0; k < ia.size(); ++k) ia[k] = edge_aux[h.ieid[k]];
    for (size_t k = 0; k < fa.size(); ++k) fa[k] = edge_aux[h.fieid[k]];
    if (ia.empty()) ia.push_back(0.0);
    if (fa.empty()) fa.push_back(0.0);
    if (int r = dev_upload(g->allocs, ia, &g->dev.iaux)) return r;
    if (int r = dev_upload(g->allocs, fa, &g->dev.fiaux)) return r;
    return SPE_OK;
}

int spe_graph_info_get(const spe_graph* g, spe_graph_info* out) {
    if (!g || !out) return fail(SPE_EINVAL, "NULL argument");
    if (out->struct_size != sizeof(spe_graph_info)) return fail(SPE_EINVAL, ABI_MSG("spe_graph_info"));
    out->n_vertices = g->hg.n;
    out->n_edges = g->hg.m;
    out->n_relax_entries = (int64_t)g->hg.icol.size();
    out->n_relax_vertices = g->hg.nc;
    out->directed = g->hg.directed;
    out->prefer_direct = g->hg.prefer_direct;
    out->complete = g->hg.complete;
    out->parallel_latency_differs = g->hg.multi_rep;
    out->weight_floor_ok = g->hg.weight_floor_ok;
    out->device = g->device;
    out->sums_exact = g->hg.share.eligible && g->hg.share.exact;
    out->shared_rows_exact = out->sums_exact && g->hg.share.prod_exact;
    return SPE_OK;
}

int spe_graph_self_path(const spe_graph* g, int32_t v, spe_entry* out) {
    if (!g || !out) return fail(SPE_EINVAL, "NULL argument");
    const spe::HostGraph& h = g->hg;
    if (v < 0 || v >= h.n) return fail(SPE_EINVAL, "vertex out of range");
    if (h.self_other[(size_t)v] < 0) {
        *out = spe_entry{-1.0, -1.0, -1, 0};
    } else {
        *out = spe_entry{h.self_w2[(size_t)v], h.self_a2[(size_t)v], h.self_other[(size_t)v], 2};
    }
    return SPE_OK;
}

int spe_graph_adjacent(const spe_graph* g, int32_t from, int32_t to, int32_t* out) {
    if (!g || !out) return fail(SPE_EINVAL, "NULL argument");
    const spe::HostGraph& h = g->hg;
    if (from < 0 || from >= h.n || to < 0 || to >= h.n) return fail(SPE_EINVAL, "vertex out of range");
    if (from == to) {   // self-loops are kept out of the CSRs (get_eid(v, v): loop_eid)
        *out = h.loop_eid[(size_t)from] >= 0 ? 1 : 0;
        return SPE_OK;
    }
    // the out-CSR of a directed graph (never pruned), the full original-id in-CSR
    // of an undirected one (symmetric: search the list of `to` for `from`)
    const std::vector<int32_t>& ptr = h.directed ? h.optr : h.fiptr;
    const std::vector<int32_t>& col = h.directed ? h.ocol : h.ficol;
    const int32_t row = h.directed ? from : to, key = h.directed ? to : from;
    *out = std::binary_search(col.begin() + ptr[(size_t)row], col.begin() + ptr[(size_t)row + 1], key) ? 1 : 0;
    return SPE_OK;
}

int spe_graph_edge(const spe_graph* g, int32_t from, int32_t to, double* latency, double* reliability) {
    if (!g) return fail(SPE_EINVAL, "NULL argument");
    const spe::HostGraph& h = g->hg;
    if (from < 0 || from >= h.n || to < 0 || to >= h.n) return fail(SPE_EINVAL, "vertex out of range");
    double w = NAN, a = NAN;
    if (from == to) {
        if (h.loop_eid[(size_t)from] >= 0) {
            w = h.loop_w[(size_t)from];
            a = h.loop_a[(size_t)from];
        }
    } else {
        const std::vector<int32_t>& ptr = h.directed ? h.optr : h.fiptr;
        const std::vector<int32_t>& col = h.directed ? h.ocol : h.ficol;
        const int32_t row = h.directed ? from : to, key = h.directed ? to : from;
        const auto b = col.begin() + ptr[(size_t)row], e = col.begin() + ptr[(size_t)row + 1];
        const auto it = std::lower_bound(b, e, key);
        if (it != e && *it == key) {
            const size_t k = (size_t)(it - col.begin());
            w = h.directed ? h.owrep[k] : h.fiwrep[k];
            a = h.directed ? h.oarep[k] : h.fia[k];
        }
    }
    if (std::isnan(w)) return fail(SPE_EINVAL, "no such edge");
    if (latency) *latency = w;
    if (reliability) *reliability = a;
    return SPE_OK;
}

int spe_order_sources(const spe_graph* g, const int32_t* attached, int32_t n_attached, int32_t* order_out) {
    if (!g || (n_attached > 0 && (!attached || !order_out))) return fail(SPE_EINVAL, "NULL argument");
    if (n_attached < 0) return fail(SPE_EINVAL, "negative n_attached");
    const spe::HostGraph& h = g->hg;
    // relaxation vertex of every source (a pruned pendant's anchor, else itself)
    std::vector<int32_t> rv((size_t)n_attached);
    std::vector<int32_t> distinct;
    for (int32_t i = 0; i < n_attached; ++i) {
        const int32_t v = attached[i];
        if (v < 0 || v >= h.n) return fail(SPE_EINVAL, "attached vertex out of range");
        rv[(size_t)i] = h.core_id[v] >= 0 ? h.core_id[v] : h.anchor_core[v];
        if (rv[(size_t)i] >= 0) distinct.push_back(rv[(size_t)i]);
    }
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    // Voronoi cells of ceil(A / 64) seeded-random centres over the relaxation
    // graph (multi-source Dijkstra on the in-CSR): a 64-source block then holds
    // sources that are close to one another, whose lanes advance in similar rounds
    const int32_t per_cell = WAVE;   // cells of 16..512 sources measured flat within +-4 % (DESIGN §4.1)
    const size_t K = std::min(distinct.size(), (size_t)((n_attached + per_cell - 1) / per_cell));
    std::vector<int32_t> cell((size_t)h.nc, INT32_MAX);
    std::vector<double> dist((size_t)h.nc, INF);
    if (K > 0 && !h.complete) {
        std::vector<int32_t> c = distinct;
        std::mt19937_64 rng(0x5eed);
        std::shuffle(c.begin(), c.end(), rng);
        using QE = std::pair<double, int32_t>;
        std::priority_queue<QE, std::vector<QE>, std::greater<QE>> pq;
        for (size_t i = 0; i < K; ++i) {
            cell[(size_t)c[i]] = (int32_t)i;
            dist[(size_t)c[i]] = 0.0;
            pq.push({0.0, c[i]});
        }
        while (!pq.empty()) {
            const QE e = pq.top();
            pq.pop();
            const int32_t x = e.second;
            if (e.first > dist[(size_t)x]) continue;
            for (int32_t k = h.iptr[(size_t)x]; k < h.iptr[(size_t)x + 1]; ++k) {
                const int32_t u = h.icol[(size_t)k];
                const double du = e.first + h.iw[(size_t)k];
                if (du < dist[(size_t)u]) {
                    dist[(size_t)u] = du;
                    cell[(size_t)u] = cell[(size_t)x];
                    pq.push({du, u});
                }
            }
        }
    }
    struct Key {
        int32_t cell;
        double d;
        int32_t r, v;
    };
    std::vector<Key> key((size_t)n_attached);
    for (int32_t i = 0; i < n_attached; ++i) {
        const int32_t r = rv[(size_t)i];
        key[(size_t)i] = r >= 0 ? Key{cell[(size_t)r], dist[(size_t)r], r, attached[i]}
                                : Key{INT32_MAX, INF, INT32_MAX, attached[i]};
    }
    std::sort(key.begin(), key.end(), [](const Key& a, const Key& b) {
        if (a.cell != b.cell) return a.cell < b.cell;
        if (a.d != b.d) return a.d < b.d;
        if (a.r != b.r) return a.r < b.r;
        return a.v < b.v;
    });
    for (int32_t i = 0; i < n_attached; ++i) order_out[i] = key[(size_t)i].v;
    return SPE_OK;
}

void spe_graph_free(spe_graph* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    for (void* p : g->allocs) (void)hipFree(p);
    delete g;
}

int spe_table_create(spe_graph* g, const int32_t* attached, int32_t n_attached, const spe_table_opts* opts,
                     spe_table** out) {
    // (the ABI guard first: nothing else of a caller built against another spe.h is read)
    if (opts && opts->struct_size != sizeof(spe_table_opts)) return fail(SPE_EINVAL, ABI_MSG("spe_table_opts"));
    if (!g || !attached || n_attached <= 0 || !out) return fail(SPE_EINVAL, "spe_table_create: bad arguments");
    *out = nullptr;
    HIP_TRY(hipSetDevice(g->device));
    const int32_t n_full = g->hg.n;
    const int32_t n = g->hg.nc;   // relaxation state is over the core
    std::vector<int32_t> vslot(n_full, -1);
    for (int32_t i = 0; i < n_attached; ++i) {
        const int32_t v = attached[i];
        if (v < 0 || v >= n_full) return fail(SPE_EINVAL, "attached vertex out of range");
        if (vslot[v] >= 0) return fail(SPE_EINVAL, "attached vertices must be unique");
        vslot[v] = i;
    }
    spe_table_opts o{};
    o.struct_size = sizeof(spe_table_opts);
    if (opts) {
        if (opts->struct_size != sizeof(spe_table_opts)) return fail(SPE_EINVAL, ABI_MSG("spe_table_opts"));
        o = *opts;
    }
    const int32_t nblk_all = (n_attached + WAVE - 1) / WAVE;
    // every argument check before the first allocation (nothing to unwind)
    if (o.block_begin != 0 || o.block_end != 0) {
        if (o.block_begin < 0 || o.block_end > nblk_all || o.block_begin > o.block_end)
            return fail(SPE_EINVAL, "block range out of bounds");
    }
    if (o.owner_rank && (o.block_begin != 0 || (o.block_end != 0 && o.block_end != nblk_all)))
        return fail(SPE_EUNSUPPORTED, "owner replay needs a table that owns every source block");
    if ((o.ext_latrel || o.ext_next_hop || o.ext_hops) && !(o.ext_latrel && o.ext_next_hop && o.ext_hops))
        return fail(SPE_EINVAL, "external storage needs all three fields");
    if (o.devices && o.n_devices < 1) return fail(SPE_EINVAL, "n_devices must be >= 1 with a device list");
    if (o.exact_delivery) {
        if (o.owner_rank) return fail(SPE_EUNSUPPORTED, "exact_delivery is not combinable with owner_rank");
        if (o.want_aux) return fail(SPE_EUNSUPPORTED, "exact_delivery is not combinable with want_aux");
        if (o.n_devices > 1) return fail(SPE_EUNSUPPORTED, "exact_delivery is not combinable with n_devices > 1");
        if (!(o.delivery_refold_max >= 0.0 && o.delivery_refold_max <= 1.0))
            return fail(SPE_EINVAL, "delivery_refold_max must lie in (0, 1] (0 = the default)");
    }
    auto* t = new spe_table();
    t->g = g;
    t->A = n_attached;
    t->attached.assign(attached, attached + n_attached);
    t->blk0 = 0;
    t->blk1 = nblk_all;
    if (o.block_begin != 0 || o.block_end != 0) {
        t->blk0 = o.block_begin;
        t->blk1 = o.block_end;
    }
    t->row_base = t->blk0;
    t->stats.replica_mismatches = -1;   // not checked (spe_table_opts.verify_replicas)
    const bool force = o.force_sssp != 0;
    {   // table cache key: graph, attached set, and every option that changes a row
        Fnv f;
        const char fmt[] = "spe-table-v1 latrel+next+hops SB64";
        f.add(fmt, sizeof(fmt));
        f.val(g->key);
        f.val(n_attached);
        f.add(attached, (size_t)n_attached * sizeof(int32_t));
        f.val(o.self_mode);
        const int32_t fs = force;
        f.val(fs);
        f.val(t->blk0);
        f.val(t->blk1);
        const int32_t has_owner = o.owner_rank != nullptr;
        f.val(has_owner);
        const int32_t aux = o.want_aux != 0;
        f.val(aux);
        const int32_t exact_src = o.exact_sources != 0;   // shared anchor trees change the last bits
        f.val(exact_src);
        if (has_owner) f.add(o.owner_rank, (size_t)n_attached * sizeof(int32_t));
        if (o.exact_delivery) {   // hashed only when set: every earlier key is unchanged
            const char ed[] = "exact_delivery";
            f.add(ed, sizeof(ed));
        }
        t->key = f.h;
    }
    if (o.devices) {   // one process, several devices (spe_multi.cpp)
        int r = spe::multi_create(g, attached, n_attached, o, &t->multi);
        if (r) {
            delete t;
            return r;
        }
        *out = t;
        return SPE_OK;
    }
    t->md.complete = g->hg.complete && !force;
    t->md.prefer = g->hg.prefer_direct && !force;
    if (o.want_aux) {   // the aux fold walks the batch engine's parent edges: SSSP rows only
        if (!g->dev.iaux) {
            delete t;
            return fail(SPE_ESTATE, "want_aux: no auxiliary edge attribute (spe_graph_set_edge_aux)");
        }
        if (t->md.complete || t->md.prefer || o.owner_rank) {
            delete t;
            return fail(SPE_EUNSUPPORTED, "want_aux needs SSSP rows (force_sssp on complete/preferdirect graphs, "
                                          "no owner replay)");
        }
        if (o.engine == SPE_ENGINE_LDS) {
            delete t;
            return fail(SPE_EUNSUPPORTED, "want_aux runs on the batch engine");
        }
        o.engine = SPE_ENGINE_BATCH;
    }
    t->md.self_mode = o.self_mode;
    t->md.multi_rep = g->hg.multi_rep;
    t->md.directed = g->hg.directed;
    // groups per launch: ~10M (group, vertex) rows per relaxation round.  Fewer,
    // larger batches cut the rounds a table takes (each batch converges in ~the
    // same count) and the near-empty tail rounds of each batch.  Same-box sweeps
    // (tools/gpu_groups_big.sh): C3 46 / 98 / 196 / 261 / 391 / 782 groups ->
    // 89-94k / 98.9k / 101.5k / 102.3k / 98.5k / 98.8k sources/s (one or two
    // batches lose the rows / relaxation overlap); C4 64 / 196 / 391 -> 278k /
    // 315k / 335k.  Batches are balanced; the state (n * 64 * 28 B per group, held
    // twice: the rows of one batch overlap the next batch's relaxation) must fit
    // the device's free HBM next to the table (the table and 4 GB kept free).
    int32_t groups = o.groups_per_launch;
    const int32_t owned = std::max(1, t->blk1 - t->blk0);
    if (groups <= 0) {
        const double per_group = 2.0 * ((double)n * WAVE * 28.0 + 4.0 * n + 2.0 * (double)g->hg.icol.size());
        double want = std::max(1.0, std::round(1.0e7 / std::max(1, n)));
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(g->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
            const bool ext = o.ext_latrel || o.ext_next_hop || o.ext_hops;
            const double rec = 22.0 + (o.owner_rank ? 4.0 : 0.0) + (o.want_aux ? 8.0 : 0.0);
            const double table_b = ext ? 0.0 : (double)owned * n_attached * WAVE * rec;
            const double ldf = std::ceil(std::max(1, n) / 64.0) * 64.0;   // FW engine: its closure, 20 B x ld^2
            const double closure_b = o.engine == SPE_ENGINE_FW ? 20.0 * ldf * ldf : 0.0;
            const double budget = (double)free_b - table_b - closure_b - 4.0e9;
            want = std::min(want, std::max(1.0, budget / per_group));
        } else {
            want = std::min(want, 6.0e9 / per_group);
        }
        const int32_t w = (int32_t)std::min<double>(want, owned);
        const int32_t batches = (owned + w - 1) / w;
        groups = (owned + batches - 1) / batches;
        if (groups > 1 && groups % 2 && groups + 1 <= w) ++groups;   // even: no padding lanes at L = 128
    }
    t->groups = std::max(1, std::min(groups, owned));
    // sources per lane group (shared frontier); 64/L groups per 64-source block
    int32_t lanes = o.lanes_per_group;
    // default: 128 sources per relaxation row (2 per thread) when every full build
    // launch covers an even or a large block count, else 64.
    // Same-box A/B, three pairs: C3 +1.4..2.1 %, C4 within +-0.5 %.
    // (an odd launch pads one block of empty lanes: 1 / (groups + 1) extra work)
    if (lanes <= 0) lanes = (t->groups >= 2 && (t->groups % 2 == 0 || t->groups >= 32)) ? 128 : 64;
    if (lanes != 64 && lanes != 128) {
        delete t;
        return fail(SPE_EINVAL, "lanes_per_group must be 64 or 128");
    }
    t->lanes = lanes;
    {
        const bool fits = lds_bytes(g->hg.nc) <= (size_t)LDS_MAX_BYTES && g->hg.nc <= LDS_VPT * LDS_T;
        int32_t e = o.engine;
        if (e == SPE_ENGINE_FW && !t->md.complete && (int64_t)g->hg.nc > FW_MAX_N) {
            delete t;
            return fail(SPE_EUNSUPPORTED, "relaxation graph too large for the FW engine (n^2 closure)");
        }
        if (e == SPE_ENGINE_LDS && !fits) {
            delete t;
            return fail(SPE_EUNSUPPORTED, "relaxation graph too large for the LDS engine");
        }
        t->engine = (e == SPE_ENGINE_AUTO) ? (fits ? SPE_ENGINE_LDS : SPE_ENGINE_BATCH) : e;
        if (t->engine == SPE_ENGINE_LDS && !t->md.complete) {
            // no HBM state: one launch covers every owned block (unless asked otherwise)
            if (o.groups_per_launch <= 0) t->groups = std::max(1, t->blk1 - t->blk0);
            const hipError_t fe = hipFuncSetAttribute((const void*)k_sssp_lds,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      (int)lds_bytes(g->hg.nc));
            if (fe != hipSuccess) {
                delete t;
                return fail(SPE_EHIP, std::string("hipFuncSetAttribute(k_sssp_lds): ") + hipGetErrorString(fe));
            }
        }
    }
    if (t->engine == SPE_ENGINE_FW) t->lanes = lanes = WAVE;   // its state walk writes 64-lane rows
    // relaxation kernel and its shape.  64 lanes: k_relax, 8 rows in flight.  128
    // lanes: k_relax_s (LDS ring, RELAX_RING_NS rows per trip) or k_relax_m (2 rows
    // in flight held to 6 waves / SIMD, MEASUREMENTS.md).  Unsupported shapes are refused.
    // (the kernel / rows / waves tuning applies to 128-lane rows; 64-lane rows run k_relax as measured)
    t->delta = o.delta_ms > 0.0 ? o.delta_ms : 0.0;
    const bool wide = lanes == 128;
    t->relax_kernel = !wide ? SPE_RELAX_REGISTER
                            : (o.relax_kernel != SPE_RELAX_AUTO ? o.relax_kernel
                                                                : (t->delta == 0.0 ? RELAX_DEFAULT_128 : SPE_RELAX_REGISTER));
    if (t->relax_kernel == SPE_RELAX_LDS_RING && t->delta > 0.0) {
        delete t;
        return fail(SPE_EUNSUPPORTED, "the LDS-ring relaxation runs 128-lane rows without the Delta schedule");
    }
    // waves_per_simd 0 = the default for the shape, 1 = the compiler's choice
    if (t->relax_kernel == SPE_RELAX_LDS_RING) {
        t->infl = o.rows_in_flight > 0 ? o.rows_in_flight : RELAX_RING_NS;
        t->occ = o.waves_per_simd > 0 ? o.waves_per_simd : (t->infl == 4 ? 8 : t->infl == 5 ? SPE_RING_OCC : t->infl == 6 ? 6 : 1);
    } else if (!wide) {
        t->infl = 8;
        t->occ = 1;
    } else {
        t->infl = o.rows_in_flight > 0 ? o.rows_in_flight : 2;
        t->occ = o.waves_per_simd > 0 ? o.waves_per_simd : (t->infl == 2 ? 6 : 1);
        if (t->delta > 0.0) {   // the Delta schedule's own instantiations
            t->infl = lanes == 64 ? 8 : 4;
            t->occ = 0;
        }
    }
    if (!relax_shape_supported(t->lanes, t->relax_kernel, t->infl, t->occ, t->delta > 0.0)) {
        delete t;
        return fail(SPE_EUNSUPPORTED, "relaxation shape (rows_in_flight, waves_per_simd) not built");
    }
    // degree-3 contraction (DESIGN §4.1): the LDS-ring batch relaxation of SSSP rows,
    // without the compat modes that walk parent edges (owner replay, aux fold)
    t->cx = g->hg.cx.active && !o.no_contract && t->engine == SPE_ENGINE_BATCH && !t->md.complete &&
            t->lanes == 128 && t->relax_kernel == SPE_RELAX_LDS_RING && t->infl == RELAX_RING_NS && t->occ == SPE_RING_OCC &&
            t->delta == 0.0 && !o.owner_rank && !o.want_aux;
    t->bG = t->cx ? &g->devx : &g->dev;
    t->bhp = t->cx ? &g->hpx : &g->hp;
    t->bn = t->cx ? g->hg.cx.nk : g->hg.nc;
    t->bm = t->cx ? (int32_t)g->hg.cx.col.size() : (int32_t)g->hg.icol.size();
    // shared anchor trees: pendant sources relax as their anchor (DESIGN §4.1)
    t->share = !o.exact_sources && g->hg.share.eligible && t->engine == SPE_ENGINE_BATCH && !t->md.complete &&
               !o.owner_rank && !o.want_aux && t->delta == 0.0;
    if (t->share) {   // some offset source: a pruned pendant, or (contracted tables) a removed vertex
        bool any = false;
        for (int32_t i = t->blk0 * WAVE; i < std::min(n_attached, t->blk1 * WAVE) && !any; ++i) {
            const int32_t c = g->hg.core_id[(size_t)attached[i]];
            any = c < 0 || (t->cx && g->hg.cx.der[(size_t)c]);
        }
        t->share = any;
    }
    // exact_delivery acts on shared rows whose sums are not exact (elsewhere every latency
    // already is the path-order fold).  Where every relaxation edge latency, pendant edges
    // included, is itself at an ns boundary, every path sum is: no fix-up is cheaper than
    // a lane per source, so the table is created as with exact_sources = 1.
    if (o.exact_delivery && t->share && !g->hg.share.exact) {
        const spe::HostGraph& h = g->hg;
        bool grid = true;
        for (size_t k = 0; k < h.iw.size() && grid; ++k) grid = delivery_near_boundary(h.iw[k], 1);
        for (int32_t v = 0; v < h.n && grid; ++v)
            if (h.core_id[(size_t)v] < 0 && h.anchor_core[(size_t)v] >= 0)
                grid = delivery_near_boundary(h.fiw[(size_t)h.fiptr[(size_t)v]], 1);
        if (grid) {
            t->share = false;
            t->dl_fallback = 1;
        } else if (t->cx && !SPE_ROWS_LM) {
            delete t;
            return fail(SPE_EUNSUPPORTED, "exact_delivery needs the lane-major derived rows (built with SPE_ROWS_LM=0)");
        } else {
            t->delivery = true;
            const double share_max = o.delivery_refold_max > 0.0 ? o.delivery_refold_max : DELIVERY_REFOLD_DEFAULT;
            const double per_block = (double)WAVE * (double)n_attached;
            t->dl_cap = (int32_t)std::min(std::min(per_block, 2.0e9), std::max(1.0, std::ceil(share_max * per_block)));
        }
    }
    t->stats.delivery_fallback = t->dl_fallback;
    t->derive = t->share && t->cx;
    if (t->share && o.groups_per_launch <= 0) {
        // lane groups per batch for shared tables: every root of the owned range in one
        // relaxation when the state fits (the rows of a contracted source read its
        // neighbours' lanes, so they must be in its batch).  Roots: each core source and
        // pendant anchor once, a contracted source none when its three neighbours are
        // roots (derived), else its own lane.  State held once (no rows overlap).
        const spe::HostGraph& h = g->hg;
        std::vector<uint8_t> isroot((size_t)std::max(1, h.nc), 0);
        int64_t roots = 0;
        const int32_t s0 = t->blk0 * WAVE, s1 = std::min(n_attached, t->blk1 * WAVE);
        for (int32_t i = s0; i < s1; ++i) {
            const int32_t v = attached[i];
            int32_t c = h.core_id[(size_t)v];
            if (c < 0) c = h.anchor_core[(size_t)v];
            else if (t->cx && h.cx.der[(size_t)c]) continue;
            if (c >= 0 && !isroot[(size_t)c]) {
                isroot[(size_t)c] = 1;
                ++roots;
            }
        }
        if (t->cx)
            for (int32_t i = s0; i < s1; ++i) {
                const int32_t c = h.core_id[(size_t)attached[i]];
                if (c < 0 || !h.cx.der[(size_t)c]) continue;
                bool all = true;
                for (int32_t k = h.cx.dptr[(size_t)c]; k < h.cx.dptr[(size_t)c + 1]; ++k)
                    all &= h.cx.dlegs[(size_t)k].ref < 0 || isroot[(size_t)h.cx.dlegs[(size_t)k].ref] != 0;
                if (!all) ++roots;
            }
        const int32_t need = (int32_t)std::max<int64_t>(1, (roots + WAVE - 1) / WAVE);
        const double per_group = (double)t->bn * WAVE * 28.0 + 4.0 * t->bn + 2.0 * std::max(1, t->bm) +
                                 (t->derive && !(SPE_ROWS_LM && SPE_LM_FUSE) ? (double)h.cx.rcore.size() * WAVE * 24.0 : 0.0) +
                                 (t->derive && SPE_ROWS_LM ? (double)lm_stride(n_attached) * WAVE * 24.0 : 0.0);
        double cap = (double)need;
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(g->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
            const bool ext = o.ext_latrel || o.ext_next_hop || o.ext_hops;
            const double table_b = ext ? 0.0 : (double)owned * n_attached * WAVE * 22.0;
            cap = std::max(1.0, ((double)free_b - table_b - 4.0e9) / per_group);
        }
        const int32_t w = (int32_t)std::min<double>(need, cap);
        const int32_t batches = (need + w - 1) / w;
        int32_t gg = (need + batches - 1) / batches;
        if (t->lanes == 128 && gg > 1 && gg % 2) ++gg;   // no padding lanes at L = 128
        t->groups = std::max(1, std::min(gg, owned));
    }
    t->trace = o.trace != 0;
    t->tb.A = n_attached;
    const size_t elems = (size_t)(t->blk1 - t->blk0) * n_attached * WAVE;
    int r = SPE_OK;
#define TRY(x)                  \
    do {                        \
        r = (x);                \
        if (r) {                \
            spe_table_free(t);  \
            return r;           \
        }                       \
    } while (0)
    if (o.ext_latrel || o.ext_next_hop || o.ext_hops) {
        t->ext = true;
        t->built = o.ext_filled != 0;
        t->tb.lr = (double2*)o.ext_latrel;
        t->tb.next = (int32_t*)o.ext_next_hop;
        t->tb.hops = (uint16_t*)o.ext_hops;
    } else {
        TRY(dev_alloc(t->allocs, &t->tb.lr, elems));
        TRY(dev_alloc(t->allocs, &t->tb.next, elems));
        TRY(dev_alloc(t->allocs, &t->tb.hops, elems));
    }
    if (o.owner_rank) {   // owner replay needs every source row in this table (checked above)
        std::vector<int32_t> rk(o.owner_rank, o.owner_rank + n_attached);
        const int32_t* tmpr = nullptr;
        TRY(dev_upload(t->allocs, rk, &tmpr));
        t->d_rank = const_cast<int32_t*>(tmpr);
        TRY(dev_alloc(t->allocs, &t->tb.prev, elems));
    }
    if (o.want_aux) TRY(dev_alloc(t->allocs, &t->tb.aux, elems));
    const std::vector<int32_t> sv(attached, attached + n_attached);
    const int32_t* tmp = nullptr;
    TRY(dev_upload(t->allocs, sv, &tmp));
    t->d_slot_vertex = const_cast<int32_t*>(tmp);
    TRY(dev_upload(t->allocs, vslot, &tmp));
    t->d_vertex_slot = const_cast<int32_t*>(tmp);
    if (!t->md.complete) {
        const spe::HostGraph& h = g->hg;
        std::vector<SlotInfo> si(n_attached);
        for (int32_t j = 0; j < n_attached; ++j) {
            const int32_t v = attached[j];
            SlotInfo& x = si[j];
            x.t = v;
            const double ft = h.vfac[v];
            x.fast = (std::isnan(ft) || ft == 1.0) ? 1 : 0;
            if (h.core_id[v] >= 0) {
                x.c = h.core_id[v];
                x.kt = -1;
                x.pw = 0.0;
                x.pa = 1.0;
            } else {
                x.c = h.anchor_core[v];
                x.kt = h.fiptr[v];
                x.pw = h.fiw[x.kt];
                x.pa = h.fia[x.kt];
            }
            // contracted tables: kept ids; a removed target reads its three neighbours
            // (c = -2 - removed index)
            if (t->cx) x.c = h.cx.kid[x.c] >= 0 ? h.cx.kid[x.c] : -2 - h.cx.rid[x.c];
            t->pend_targets |= x.kt >= 0;
        }
        const SlotInfo* tsi = nullptr;
        TRY(dev_upload(t->allocs, si, &tsi));
        t->d_slots = const_cast<SlotInfo*>(tsi);
    }
    if (!t->md.complete && t->engine == SPE_ENGINE_LDS) {
        const spe::HostGraph& h = g->hg;
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device);
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, LDS_MAX_BYTES / lds_bytes(h.nc)));
        t->lds_grid = cus * per_cu;
        const size_t per = (size_t)t->lds_grid * std::max(1, h.nc);
        TRY(dev_alloc(t->allocs, &t->lsc.par, per));
    }
    const size_t G = (size_t)t->groups;
    // lane groups per batch (L > 64: a group spans L / 64 blocks; an odd tail is padded)
    const size_t GL = t->lanes <= WAVE ? G * (WAVE / t->lanes) : (G * WAVE + t->lanes - 1) / t->lanes;
    const size_t GW = GL * (size_t)t->lanes;   // source entries per batch (>= G * 64: padding lanes)
    if (!t->md.complete && t->engine == SPE_ENGINE_BATCH) {
        const size_t se = GW * (size_t)t->bn;
        // (shared tables relax and write rows on one stream: one state buffer)
        t->overlap = o.no_overlap == 0 && !t->share;
        for (int i = 0; i < (t->overlap ? 2 : 1); ++i) {
            TRY(dev_alloc(t->allocs, &t->st_buf[i].D, se));
            TRY(dev_alloc(t->allocs, &t->st_buf[i].P, se));
            TRY(dev_alloc(t->allocs, &t->st_buf[i].RT, se));
        }
        t->st = t->st_buf[0];
        const size_t nrel = std::max<size_t>(1, (size_t)t->bm);
        TRY(dev_alloc(t->allocs, &t->inflag[0], GL * nrel));
        TRY(dev_alloc(t->allocs, &t->inflag[1], GL * nrel));
        TRY(dev_alloc(t->allocs, &t->mark[0], (GL * t->bn + 8) & ~(size_t)7));
        TRY(dev_alloc(t->allocs, &t->mark[1], (GL * t->bn + 8) & ~(size_t)7));
        TRY(dev_alloc(t->allocs, &t->hmark[0], GL * t->bn));
        TRY(dev_alloc(t->allocs, &t->hmark[1], GL * t->bn));
        const size_t pe = GW * std::max<size_t>(1, (size_t)t->bhp->nseg);
        TRY(dev_alloc(t->allocs, &t->pp.alt, pe));
        TRY(dev_alloc(t->allocs, &t->pp.du, pe));
        TRY(dev_alloc(t->allocs, &t->pp.uk, pe));
        if (t->share && SPE_MARGIN_ONLINE) {   // shared tables: the online margin proof (k_tight_reduce)
            TRY(dev_alloc(t->allocs, &t->pp.tg, pe));
            TRY(dev_alloc(t->allocs, &t->tight, GL * (size_t)t->bn * 2));
        }
        t->max_iters = 4 * t->bn + 64;
        TRY(dev_alloc(t->allocs, &t->counts, (size_t)t->max_iters + 2));
        if (SPE_ROUTE_PASS && t->relax_kernel == SPE_RELAX_LDS_RING && t->lanes == 2 * WAVE) {
            for (int i = 0; i < 2; ++i) TRY(dev_alloc(t->allocs, &t->rpend[i], GL * (size_t)t->bn * 2));
            TRY(dev_alloc(t->allocs, &t->rcounts, (size_t)t->max_iters + 2));
        }
        for (int i = 0; i < 3; ++i) TRY(dev_alloc(t->allocs, &t->fbound[i], GW));
        if (SPE_RELAX_STATS) TRY(dev_alloc(t->allocs, &t->rstats, ((size_t)t->max_iters + 2) * RS_N));
        if (t->delta > 0.0) {
            t->max_iters = 64 * t->bn + 4096;   // buckets add rounds
            TRY(dev_alloc(t->allocs, &t->counts, (size_t)t->max_iters + 2));
            TRY(dev_alloc(t->allocs, &t->ds.bound, GL));
            TRY(dev_alloc(t->allocs, &t->ds.minrej, GL));
            TRY(dev_alloc(t->allocs, &t->ds.gchanged, GL));
            TRY(dev_alloc(t->allocs, &t->ds.pending, GL * t->bn));
        }
    }
    if (!t->md.complete && t->engine == SPE_ENGINE_FW) {
        const size_t se = GW * n;
        TRY(dev_alloc(t->allocs, &t->st_buf[0].D, se));
        TRY(dev_alloc(t->allocs, &t->st_buf[0].P, se));
        TRY(dev_alloc(t->allocs, &t->st_buf[0].RT, se));
        t->st = t->st_buf[0];
        t->fw_ld = ((int64_t)std::max(1, n) + FWB - 1) / FWB * FWB;
        const size_t ll = (size_t)t->fw_ld * (size_t)t->fw_ld;
        TRY(dev_alloc(t->allocs, &t->fw.D, ll));
        if (getenv("SPE_FW_TRIPLE")) TRY(dev_alloc(t->allocs, &t->fw.R, ll));   // else the (D, N) closure: rows re-fold R
        TRY(dev_alloc(t->allocs, &t->fw.N, ll));
    }
    for (int i = 0; i < (t->overlap ? 2 : 1); ++i) {
        TRY(dev_alloc(t->allocs, &t->srcv_buf[i], GW));
        TRY(dev_alloc(t->allocs, &t->srcc_buf[i], GW));
    }
    t->d_srcv = t->srcv_buf[0];
    t->d_srcc = t->srcc_buf[0];
    TRY(dev_alloc(t->allocs, &t->d_min, 1));
    const size_t owned_slots = (size_t)std::max(1, t->blk1 - t->blk0) * WAVE;
    if (t->share) {
        for (int i = 0; i < (t->overlap ? 2 : 1); ++i) {
            TRY(dev_alloc(t->allocs, &t->rsrc_buf[i], owned_slots));
            TRY(dev_alloc(t->allocs, &t->rli_buf[i], owned_slots));
            TRY(dev_alloc(t->allocs, &t->rwa_buf[i], owned_slots));
            TRY(dev_alloc(t->allocs, &t->rng_buf[i], owned_slots / WAVE / RT_B + 2));
        }
        TRY(dev_alloc(t->allocs, &t->d_unsafe, GW));
        if (t->derive) {
            int32_t ml = 1;
            for (size_t c = 0; c + 1 < g->hg.cx.dptr.size(); ++c)
                ml = std::max(ml, g->hg.cx.dptr[c + 1] - g->hg.cx.dptr[c]);
            t->leg_cap = owned_slots * (size_t)ml;
            TRY(dev_alloc(t->allocs, &t->d_der, t->leg_cap));
            TRY(dev_alloc(t->allocs, &t->d_sunsafe, owned_slots));
            const spe::HostGraph& h = g->hg;
            t->nr = (int32_t)h.cx.rcore.size();
            // (the lane-major staging expands removed targets itself: no DX / RTX)
            const size_t sx = SPE_ROWS_LM && SPE_LM_FUSE ? 1 : GW * (size_t)std::max(1, t->nr);
            TRY(dev_alloc(t->allocs, &t->d_dx, sx));
            TRY(dev_alloc(t->allocs, &t->d_rtx, sx));
            if (SPE_ROWS_LM) {   // lane-major staging: every root lane at every target slot
                const size_t sl = GW * (size_t)lm_stride(n_attached);
                TRY(dev_alloc(t->allocs, &t->d_xd, sl));
                TRY(dev_alloc(t->allocs, &t->d_xrt, sl));
            }
            std::vector<int32_t> ro((size_t)std::max(1, t->nr), -1);
            for (int32_t r = 0; r < t->nr; ++r) ro[(size_t)r] = h.corev[(size_t)h.cx.rcore[(size_t)r]];
            TRY(dev_upload(t->allocs, ro, &t->d_rorig));
        }
        if (t->delivery) {   // the worklist: the sum of the block caps of the largest batch (every owned block)
            TRY(dev_alloc(t->allocs, &t->d_dlcnt, 2 * (owned_slots / WAVE)));   // flagged, then changed
            TRY(dev_alloc(t->allocs, &t->d_dlwork, owned_slots / WAVE * (size_t)t->dl_cap));
        }
    }
#undef TRY
    // every failure from here on releases what was allocated (spe_table_free)
#define HTRY(expr)                                                                         \
    do {                                                                                   \
        const hipError_t _e = (expr);                                                      \
        if (_e != hipSuccess) {                                                            \
            spe_table_free(t);                                                             \
            return fail(SPE_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
        }                                                                                  \
    } while (0)
    HTRY(hipHostMalloc((void**)&t->h_srcv, 2 * GW * sizeof(int32_t), hipHostMallocDefault));
    if (t->share) {
        HTRY(hipHostMalloc((void**)&t->h_rows,
                           owned_slots * (sizeof(double2) + sizeof(int2) + sizeof(int32_t)) +
                               (owned_slots / WAVE / RT_B + 2) * sizeof(int2),
                           hipHostMallocDefault));
        HTRY(hipHostMalloc((void**)&t->h_unsafe, GW, hipHostMallocDefault));
        if (t->derive) {
            HTRY(hipHostMalloc((void**)&t->h_der, t->leg_cap * sizeof(DLeg), hipHostMallocDefault));
            HTRY(hipHostMalloc((void**)&t->h_sunsafe, owned_slots, hipHostMallocDefault));
        }
        if (t->delivery) {
            HTRY(hipHostMalloc((void**)&t->h_dl, 2 * (owned_slots / WAVE) * sizeof(uint32_t), hipHostMallocDefault));
            HTRY(hipEventCreate(&t->ev_dl[0]));
            HTRY(hipEventCreate(&t->ev_dl[1]));
        }
    }
    HTRY(hipHostMalloc((void**)&t->h_counts, std::max<size_t>(64, (size_t)t->max_iters + 2) * sizeof(int32_t),
                       hipHostMallocDefault));
    HTRY(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    if (t->overlap) {
        HTRY(hipStreamCreateWithFlags(&t->rows_stream, hipStreamNonBlocking));
        HTRY(hipEventCreateWithFlags(&t->ev_relaxed, hipEventDisableTiming));
        HTRY(hipEventCreateWithFlags(&t->ev_rows[0], hipEventDisableTiming));
        HTRY(hipEventCreateWithFlags(&t->ev_rows[1], hipEventDisableTiming));
    }
#undef HTRY
    t->blk_built.assign((size_t)(t->blk1 - t->blk0), t->built ? 1 : 0);
    *out = t;
    return SPE_OK;
}

// Event bracketing around a launch (no-op unless profiling is enabled).
struct LaunchTimer {
    spe_table* t;
    hipStream_t s;
    int kind;
    hipEvent_t a = nullptr, b = nullptr;
    LaunchTimer(spe_table* t_, hipStream_t s_, int kind_) : t(t_), s(s_), kind(kind_) {
        if (!t->prof) return;
        if (t->ev_next + 2 > t->ev_pool.size()) {
            for (int i = 0; i < 256; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) return;
                t->ev_pool.push_back(e);
            }
        }
        a = t->ev_pool[t->ev_next++];
        b = t->ev_pool[t->ev_next++];
        (void)hipEventRecord(a, s);
    }
    ~LaunchTimer() {
        if (!a) return;
        (void)hipEventRecord(b, s);
        t->pending.push_back({kind, a, b});
    }
};

// all = false: only records whose end event has completed (the rows stream may
// still run); the pool is recycled once nothing is pending.
static int resolve_profile(spe_table* t, bool all = true) {
    std::vector<spe_table::Rec> keep;
    for (auto& r : t->pending) {
        if (!all && hipEventQuery(r.b) != hipSuccess) {
            keep.push_back(r);
            continue;
        }
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        t->kp.ms[r.kind] += ms;
        t->kp.launches[r.kind] += 1;
        if (t->trace) fprintf(stderr, "spe-trace %d %.4f\n", r.kind, ms);
    }
    t->pending.swap(keep);
    if (t->pending.empty()) t->ev_next = 0;
    return SPE_OK;
}

extern "C++" {
// The FW engine's closure (D, R, N) over the relaxation graph, ld x ld, enqueued on s.
// M.R == NULL: the pair (D, N) only (table builds: the rows re-fold reliability).
static int fw3_closure(const spe_graph* g, Fw3 M, int64_t ld, hipStream_t s) {
    const int32_t nb = (int32_t)(ld / FWB);
    const bool wr = M.R != nullptr;
    HIP_TRY(hipFuncSetAttribute(wr ? (const void*)k_fw3_panel<true> : (const void*)k_fw3_panel<false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, FW3_LDS));
    HIP_TRY(hipFuncSetAttribute(wr ? (const void*)k_fw3_rest<true> : (const void*)k_fw3_rest<false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, wr ? FW3_REST_LDS : FW2_REST_LDS));
    k_fw3_init<<<grid_for(ld * ld, 256, 16384), 256, 0, s>>>(ld, M);
    const int32_t nrel = (int32_t)g->hg.icol.size();
    if (nrel > 0) k_fw3_edges<<<(nrel + 255) / 256, 256, 0, s>>>(nrel, ld, g->dev, M);
    // padding rows / columns stay +inf off the diagonal: they never shorten a path
    for (int32_t kb = 0; kb < nb; ++kb) {
        if (wr) {
            k_fw3_panel<true><<<1, 256, FW3_LDS, s>>>(kb, nb, ld, M, 0, 0, nb);
            if (nb > 1) k_fw3_panel<true><<<2 * nb - 2, 256, FW3_LDS, s>>>(kb, nb, ld, M, 1, 0, nb);
            if (nb > 1) k_fw3_rest<true><<<(nb - 1) * (nb - 1), 256, FW3_REST_LDS, s>>>(kb, nb, ld, M, 0, nb);
        } else {
            k_fw3_panel<false><<<1, 256, FW3_LDS, s>>>(kb, nb, ld, M, 0, 0, nb);
            if (nb > 1) k_fw3_panel<false><<<2 * nb - 2, 256, FW3_LDS, s>>>(kb, nb, ld, M, 1, 0, nb);
            if (nb > 1) k_fw3_rest<false><<<(nb - 1) * (nb - 1), 256, FW2_REST_LDS, s>>>(kb, nb, ld, M, 0, nb);
        }
    }
    HIP_TRY(hipGetLastError());
    return SPE_OK;
}

