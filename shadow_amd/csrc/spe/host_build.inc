// host_build.inc -- part of spe.hip (one translation unit).
// Host side: table builds -- the relaxation loop, batch scheduling, shared anchor
// trees and derived rows, the LDS / FW engines, the multi-device FW closure.

// ---- the multi-device FW closure (spe_multi.cpp drives it; SURVEY §8e): 1-D
// row blocks per device; per pivot block the owner relaxes the diagonal tile and
// the pivot row panel, the panel is broadcast, and every device relaxes its own
// rows' column panel and remaining tiles.
namespace spe {
int fw_part(spe_table* t, FwPart* out) {
    if (!t || t->engine != SPE_ENGINE_FW || t->md.complete || !t->fw.D) return set_error(SPE_EINVAL, "not an FW-engine table");
    out->D = t->fw.D;
    out->R = t->fw.R;
    out->N = t->fw.N;
    out->ld = t->fw_ld;
    out->device = t->g->device;
    out->stream = t->stream;
    out->done = &t->fw_done;
    return SPE_OK;
}
int fw_init(const spe_graph* g, const FwPart& p) {
    HIP_TRY(hipSetDevice(p.device));
    for (const void* f : {(const void*)k_fw3_panel<true>, (const void*)k_fw3_panel<false>})
        HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, FW3_LDS));
    HIP_TRY(hipFuncSetAttribute((const void*)k_fw3_rest<true>, hipFuncAttributeMaxDynamicSharedMemorySize, FW3_REST_LDS));
    HIP_TRY(hipFuncSetAttribute((const void*)k_fw3_rest<false>, hipFuncAttributeMaxDynamicSharedMemorySize, FW2_REST_LDS));
    hipStream_t s = (hipStream_t)p.stream;
    const Fw3 M{p.D, p.R, p.N};
    k_fw3_init<<<grid_for(p.ld * p.ld, 256, 16384), 256, 0, s>>>(p.ld, M);
    const int32_t nrel = (int32_t)g->hg.icol.size();
    if (nrel > 0) k_fw3_edges<<<(nrel + 255) / 256, 256, 0, s>>>(nrel, p.ld, g->dev, M);
    HIP_TRY(hipGetLastError());
    return SPE_OK;
}
int fw_pivot_owner(const FwPart& p, int32_t kb) {
    HIP_TRY(hipSetDevice(p.device));
    const int32_t nb = (int32_t)(p.ld / FWB);
    hipStream_t s = (hipStream_t)p.stream;
    const Fw3 M{p.D, p.R, p.N};
    if (p.R) {
        k_fw3_panel<true><<<1, 256, FW3_LDS, s>>>(kb, nb, p.ld, M, 0, 0, nb);
        if (nb > 1) k_fw3_panel<true><<<nb - 1, 256, FW3_LDS, s>>>(kb, nb, p.ld, M, 1, 0, nb);   // row panel only
    } else {
        k_fw3_panel<false><<<1, 256, FW3_LDS, s>>>(kb, nb, p.ld, M, 0, 0, nb);
        if (nb > 1) k_fw3_panel<false><<<nb - 1, 256, FW3_LDS, s>>>(kb, nb, p.ld, M, 1, 0, nb);
    }
    HIP_TRY(hipGetLastError());
    return SPE_OK;
}
int fw_pivot_rows(const FwPart& p, int32_t kb, int32_t rb0, int32_t rb1) {
    HIP_TRY(hipSetDevice(p.device));
    const int32_t nb = (int32_t)(p.ld / FWB);
    const int32_t rows = (rb1 - rb0) - ((kb >= rb0 && kb < rb1) ? 1 : 0);
    if (rows <= 0 || nb < 2) return SPE_OK;
    hipStream_t s = (hipStream_t)p.stream;
    const Fw3 M{p.D, p.R, p.N};
    if (p.R) {
        k_fw3_panel<true><<<rows, 256, FW3_LDS, s>>>(kb, nb, p.ld, M, nb, rb0, rb1);   // column panel, own rows
        k_fw3_rest<true><<<rows * (nb - 1), 256, FW3_REST_LDS, s>>>(kb, nb, p.ld, M, rb0, rb1);
    } else {
        k_fw3_panel<false><<<rows, 256, FW3_LDS, s>>>(kb, nb, p.ld, M, nb, rb0, rb1);
        k_fw3_rest<false><<<rows * (nb - 1), 256, FW2_REST_LDS, s>>>(kb, nb, p.ld, M, rb0, rb1);
    }
    HIP_TRY(hipGetLastError());
    return SPE_OK;
}
}  // namespace spe

// The route pass (SPE_ROUTE_PASS, kernels_relax.inc): k_routes_init marks every lane
// with a parent entry pending, then one k_routes launch per tree level.  Launches are
// enqueued in chunks sized by the previous batch's level count; levels after the last
// exit at once (rcounts: 1 while some lane is pending).
static int routes_to_completion(spe_table* t, int32_t groups, hipStream_t s) {
    const int32_t n = t->bn;
    const int64_t items = (int64_t)groups * n;
    if (!t->rpend[0] || !t->rcounts) return fail(SPE_ESTATE, "route pass buffers missing");
    const DevGraph& G = *t->bG;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_routes<true>, BLOCK, 0) != hipSuccess ||
        per_cu < 1)
        per_cu = 4;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->g->device) != hipSuccess || cus < 1)
        cus = 256;
    const int grid = (grid_for((items + WAVE - 1) / WAVE * WAVE, BLOCK, per_cu * cus) + 7) & ~7;
    HIP_TRY(hipMemsetAsync(t->rcounts, 0, sizeof(int32_t) * ((size_t)t->max_iters + 2), s));
    {
        LaunchTimer lt(t, s, SPE_K_ROUTES);
        const int64_t elems = items * 2 * WAVE;
        k_routes_init<<<grid_for(elems, BLOCK, 8192), BLOCK, 0, s>>>(elems, t->st.P, t->rpend[0], t->rcounts);
    }
    int32_t r = 1;
    int32_t chunk = t->last_route_rounds > 0 ? t->last_route_rounds + 1 : 16;
    for (;;) {
        for (int32_t q = 0; q < chunk; ++q, ++r) {
            if (r > t->max_iters) {
                if (getenv("SPE_ROUTE_DEBUG")) {   // the first stuck lanes: entry, parent, the parent's state
                    const size_t words = (size_t)items * 2;
                    std::vector<unsigned long long> pw(words);
                    std::vector<int32_t> P((size_t)items * 2 * WAVE);
                    std::vector<int32_t> icol((size_t)std::max(1, t->bm));
                    (void)hipMemcpy(pw.data(), t->rpend[(r - 1) & 1], words * 8, hipMemcpyDeviceToHost);
                    (void)hipMemcpy(P.data(), t->st.P, P.size() * 4, hipMemcpyDeviceToHost);
                    (void)hipMemcpy(icol.data(), G.icol, icol.size() * 4, hipMemcpyDeviceToHost);
                    int shown = 0;
                    for (size_t w = 0; w < words && shown < 8; ++w)
                        for (int l = 0; l < WAVE && shown < 8; ++l)
                            if ((pw[w] >> l) & 1ull) {
                                const int64_t item = (int64_t)(w >> 1);
                                const int32_t g = (int32_t)(item / n), v = (int32_t)(item % n);
                                const int32_t k = P[w * WAVE + l], u = k >= 0 ? icol[k] : -9;
                                const size_t pwu = 2 * ((size_t)g * n + (size_t)u) + (w & 1);
                                fprintf(stderr, "spe-route-debug word %zu g %d v %d lane %d P %d u %d parent_pending %d parent_P %d\n",
                                        w, g, v, (int)((w & 1) * WAVE + l), k, u, u >= 0 ? (int)((pw[pwu] >> l) & 1ull) : -1,
                                        u >= 0 ? P[pwu * WAVE + l] : -9);
                                ++shown;
                                if (shown == 1) {   // the first stuck lane's parent chain
                                    std::vector<double> D((size_t)items * 2 * WAVE);
                                    (void)hipMemcpy(D.data(), t->st.D, D.size() * 8, hipMemcpyDeviceToHost);
                                    const int32_t j = (int32_t)((w & 1) * WAVE + l);
                                    int32_t x = v;
                                    for (int step = 0; step < 24 && x >= 0; ++step) {
                                        const size_t e = ((size_t)g * n + (size_t)x) * 2 * WAVE + (size_t)j;
                                        const int32_t kx = P[e];
                                        const size_t pwx = 2 * ((size_t)g * n + (size_t)x) + (size_t)(j >= WAVE);
                                        fprintf(stderr, "spe-route-debug   chain %d: v %d D %.17g P %d pending %d\n", step, x,
                                                D[e], kx, (int)((pw[pwx] >> (j & (WAVE - 1))) & 1ull));
                                        x = kx >= 0 ? icol[kx] : -1;
                                    }
                                }
                            }
                }
                return fail(SPE_ESTATE, "route pass did not complete");
            }
            LaunchTimer lt(t, s, SPE_K_ROUTES);
            if (t->cx)
                k_routes<true><<<grid, BLOCK, 0, s>>>(items, n, t->d_srcc, G, t->st, t->rpend[(r - 1) & 1],
                                                      t->rpend[r & 1], t->rcounts + r - 1, t->rcounts + r);
            else
                k_routes<false><<<grid, BLOCK, 0, s>>>(items, n, t->d_srcc, G, t->st, t->rpend[(r - 1) & 1],
                                                       t->rpend[r & 1], t->rcounts + r - 1, t->rcounts + r);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(t->h_counts, t->rcounts, sizeof(int32_t) * (size_t)r, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (t->h_counts[r - 1] == 0) break;
        chunk = 4;
    }
    int32_t levels = 1;   // the first launch that left nothing pending
    while (levels < r && t->h_counts[levels] != 0) ++levels;
    t->last_route_rounds = levels;
    return SPE_OK;
}

template <int L, int INFL, int OCC = 1, bool DELTA = false, bool RING = false>
static int relax_to_convergence_l(spe_table* t, int32_t blocks, hipStream_t s) {
    static_assert(!RING || (L == 2 * WAVE && !DELTA), "the LDS-ring kernel runs 128-lane rows, no Delta schedule");
    constexpr int M = L > WAVE ? L / WAVE : 1;    // lanes per thread
    const spe_graph* g = t->g;
    const int32_t n = t->bn;      // the batch engine's relaxation graph (core or contracted)
    const int32_t nrel = t->bm;
    const DevGraph& G = *t->bG;
    const HeavyPlan& HP = *t->bhp;
    const int32_t groups = M > 1 ? (blocks + M - 1) / M : blocks * (WAVE / L);    // lane groups
    const int64_t total = (int64_t)groups * n;
    // one resident wave per hardware slot (no second wave of late blocks), multiple of 8 (XCD split)
    int per_cu = 0, cus = 0;
    const void* kfn;
    if constexpr (RING) kfn = t->cx ? (const void*)k_relax_s<INFL, OCC, true> : (const void*)k_relax_s<INFL, OCC>;
    else if constexpr (M > 1) kfn = (const void*)k_relax_m<M, INFL, OCC, DELTA>;
    else kfn = (const void*)k_relax<L, INFL, OCC, DELTA>;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, BLOCK, 0) != hipSuccess || per_cu < 1)
        per_cu = 4;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess || cus < 1) cus = 256;
    const int relax_grid = (grid_for((total + 7) / 8 * WAVE, BLOCK, per_cu * cus) + 7) & ~7;
    HIP_TRY(hipMemsetAsync(t->counts, 0, sizeof(int32_t) * ((size_t)t->max_iters + 2), s));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)t->counts, 1, 1, s));   // round 0 (the sources) changed
    for (int i = 0; i < 2; ++i) {   // consumers clear what they read; this only guards a failed batch
        HIP_TRY(hipMemsetAsync(t->inflag[i], 0, (size_t)groups * std::max(1, nrel) * sizeof(inflag_t), s));
        HIP_TRY(hipMemsetAsync(t->mark[i], 0, ((size_t)total + 8) & ~(size_t)7, s));
        HIP_TRY(hipMemsetAsync(t->hmark[i], 0, (size_t)total, s));
    }
    {
        LaunchTimer lt(t, s, SPE_K_INIT);
        const dim3 ig(grid_for((int64_t)n * L, BLOCK, std::max(8, 16384 / std::max(1, (int)groups))), groups);
        k_init_state<L><<<ig, BLOCK, 0, s>>>(n, groups, t->d_srcv, G.vfac, G, t->st);
    }
    if constexpr (DELTA) {
        HIP_TRY(hipMemsetAsync(t->ds.pending, 0x7F, sizeof(double) * (size_t)total, s));   // 1.4e306: none
        k_delta_init<<<(groups + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(groups, t->delta, t->ds);
    }
    // settle bounds: round 1's is 0 (the seeds' values are >= 0), round 1's changes start empty
    const bool settle = SPE_SETTLE && RING && t->fbound[0] != nullptr;
    if (settle) {
        HIP_TRY(hipMemsetAsync(t->fbound[1], 0, sizeof(unsigned long long) * (size_t)groups * L, s));
        HIP_TRY(hipMemsetAsync(t->fbound[2], 0x7F, sizeof(unsigned long long) * (size_t)groups * L, s));
    }
    if (t->rstats) HIP_TRY(hipMemsetAsync(t->rstats, 0, sizeof(unsigned long long) * ((size_t)t->max_iters + 2) * RS_N, s));
    // online margin proof: the light ring kernel and the 128-lane heavy passes carry it
    const bool track = RING && t->mg_track && t->tight != nullptr && t->pp.tg != nullptr;
    if (track) HIP_TRY(hipMemsetAsync(t->tight, 0, sizeof(unsigned long long) * (size_t)groups * n * 2, s));
    {
        LaunchTimer lt(t, s, SPE_K_SEED);
        // the sources "changed in round 0": their out-edges form round 1's frontier
        // (Delta: heavy vertices stay in the light frontier, relaxed by the same kernel)
        k_seed<L><<<(int)(((int64_t)groups * L * WAVE + BLOCK - 1) / BLOCK), BLOCK, 0, s>>>(n, groups, t->d_srcv, G, t->mark[1],
                                                                     DELTA ? t->mark[1] : t->hmark[1], t->inflag[1]);
    }
    const int64_t subs_per_wave = M > 1 ? 1 : WAVE / L;
    // the LDS-ring relaxation settles distances and parents; the route pass folds the records
    constexpr bool NORT = RING && SPE_ROUTE_PASS;
    // Rounds are enqueued in chunks sized by the previous batch's round count
    // (batches of one graph converge in similar counts); rounds after the
    // converged one exit at once, so one host check per batch is typical.
    int32_t it = 1;
    int32_t chunk = t->last_rounds > 0 ? t->last_rounds + 1 : 8;
    for (;;) {
        for (int32_t q = 0; q < chunk; ++q, ++it) {
            if (it > t->max_iters) return fail(SPE_ESTATE, "relaxation did not converge");
            Flags fl{t->mark[it & 1],   t->mark[(it + 1) & 1],   t->hmark[it & 1],
                     t->hmark[(it + 1) & 1], t->inflag[it & 1], t->inflag[(it + 1) & 1], t->counts + it,
                     t->counts + it - 1};
            if (settle) {   // round it reads buffer it % 3, writes (it + 1) % 3, resets (it + 2) % 3
                fl.fb_cur = t->fbound[it % 3];
                fl.fb_next = t->fbound[(it + 1) % 3];
                fl.fb_reset = t->fbound[(it + 2) % 3];
                fl.fb_elems = (int64_t)groups * L;
            }
            fl.rstats = t->rstats ? t->rstats + (size_t)it * RS_N : nullptr;
            fl.round = it;
            if (track) {
                fl.tight = t->tight;
                fl.mg_invw = t->mg_invw;
                fl.mg_omax = t->mg_omax;
                fl.mg_hmax = t->mg_hmax;
            }
            if constexpr (DELTA) fl.hmark_next = fl.mark_next;   // heavy rows relaxed by k_relax too
            {
                LaunchTimer lt(t, s, SPE_K_RELAX);
                if constexpr (RING) {
                    if (t->cx && track)
                        k_relax_s<INFL, OCC, true, true><<<relax_grid, BLOCK, 0, s>>>((int32_t)total, n, t->d_srcc, G, t->st, fl);
                    else if (t->cx)
                        k_relax_s<INFL, OCC, true><<<relax_grid, BLOCK, 0, s>>>((int32_t)total, n, t->d_srcc, G, t->st, fl);
                    else if (track)
                        k_relax_s<INFL, OCC, false, true><<<relax_grid, BLOCK, 0, s>>>((int32_t)total, n, t->d_srcc, G, t->st, fl);
                    else
                        k_relax_s<INFL, OCC><<<relax_grid, BLOCK, 0, s>>>((int32_t)total, n, t->d_srcc, G, t->st, fl);
                }
                else if constexpr (M > 1)
                    k_relax_m<M, INFL, OCC, DELTA><<<relax_grid, BLOCK, 0, s>>>((int32_t)total, n, t->d_srcc, G,
                                                                                t->st, fl, t->ds);
                else
                    k_relax<L, INFL, OCC, DELTA><<<relax_grid, BLOCK, 0, s>>>((int32_t)total, n, t->d_srcc, G,
                                                                              t->st, fl, t->ds);
            }
            if constexpr (DELTA) {
                k_delta_advance<<<groups, BLOCK, 0, s>>>(n, nrel, t->delta, G, t->ds, fl.mark_next, fl.in_next,
                                                         t->counts + it);
            } else if (HP.nheavy > 0) {
                LaunchTimer lt(t, s, SPE_K_HEAVY);
                const int64_t pw = ((int64_t)groups * HP.nseg + subs_per_wave - 1) / subs_per_wave;
                const int64_t cw = ((int64_t)groups * HP.nheavy + subs_per_wave - 1) / subs_per_wave;
                if constexpr (M > 1) {
                    const int pg = grid_for(pw * WAVE, BLOCK, 4096), cg = grid_for(cw * WAVE, BLOCK, 4096);
                    if (t->cx && track) {
                        k_heavy_partial_m<M, SPE_HEAVY_CX_INFL, true, true><<<pg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                        k_heavy_combine_m<M, true, true, NORT><<<cg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                    } else if (t->cx) {
                        k_heavy_partial_m<M, SPE_HEAVY_CX_INFL, true><<<pg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                        k_heavy_combine_m<M, true, false, NORT><<<cg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                    } else if (track) {
                        k_heavy_partial_m<M, INFL, false, true><<<pg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                        k_heavy_combine_m<M, false, true, NORT><<<cg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                    } else {
                        k_heavy_partial_m<M, INFL><<<pg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                        k_heavy_combine_m<M, false, false, NORT><<<cg, BLOCK, 0, s>>>(groups, n, t->d_srcc, G, t->st, HP, t->pp, fl);
                    }
                } else {
                    k_heavy_partial<L><<<grid_for(pw * WAVE, BLOCK, 4096), BLOCK, 0, s>>>(groups, n, t->d_srcc, G,
                                                                                          t->st, HP, t->pp, fl);
                    k_heavy_combine<L><<<grid_for(cw * WAVE, BLOCK, 4096), BLOCK, 0, s>>>(groups, n, t->d_srcc, G,
                                                                                          t->st, HP, t->pp, fl);
                }
            }
        }
        HIP_TRY(hipMemcpyAsync(t->h_counts, t->counts, sizeof(int32_t) * (size_t)it, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        t->stats.launches += chunk;
        if (t->h_counts[it - 1] == 0) break;
        chunk = 2;
    }
    // the first round that changed nothing ends the relaxation (work accounting)
    int32_t rounds = 1;
    while (rounds < it && t->h_counts[rounds] != 0) ++rounds;
    if (t->rstats) {   // diagnostic builds: the per-round histogram on stderr
        std::vector<unsigned long long> h((size_t)(rounds + 1) * RS_N);
        HIP_TRY(hipMemcpy(h.data(), t->rstats, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int32_t r = 1; r <= rounds; ++r) {
            const unsigned long long* c = &h[(size_t)r * RS_N];
            fprintf(stderr, "spe-relax-stats groups %d n %d round %d items %llu entries %llu lines %llu kept %llu "
                            "lanes_changed %llu items_changed %llu\n", groups, n, r, c[RS_ITEMS], c[RS_ENTRIES],
                    c[RS_LINES], c[RS_LINES_KEPT], c[RS_LANES_CHANGED], c[RS_ITEMS_CHANGED]);
        }
    }
    t->stats.active_rounds += rounds - 1;
    t->stats.iterations += rounds;
    t->last_rounds = rounds;
    if constexpr (NORT) return routes_to_completion(t, groups, s);
    return SPE_OK;
}

static int relax_to_convergence(spe_table* t, int32_t blocks, hipStream_t s) {
    if (t->delta > 0.0)   // measured slower (MEASUREMENTS.md)
        return t->lanes == 128 ? relax_to_convergence_l<128, 4, 1, true>(t, blocks, s)
                               : relax_to_convergence_l<64, 8, 1, true>(t, blocks, s);
    if (t->lanes == 64) return relax_to_convergence_l<64, 8>(t, blocks, s);
    if (t->relax_kernel == SPE_RELAX_LDS_RING) {
        if (t->infl == 4) return relax_to_convergence_l<128, 4, 8, false, true>(t, blocks, s);
        if (t->infl == 6) return relax_to_convergence_l<128, 6, 6, false, true>(t, blocks, s);
        return relax_to_convergence_l<128, 5, SPE_RING_OCC, false, true>(t, blocks, s);
    }
    if (t->infl == 4) return relax_to_convergence_l<128, 4>(t, blocks, s);
    return t->occ == 6 ? relax_to_convergence_l<128, 2, 6>(t, blocks, s) : relax_to_convergence_l<128, 2>(t, blocks, s);
}

static void launch_rows_sssp(spe_table* t, int grid, int32_t blocks, int32_t sb0, hipStream_t s) {
#define ROWS(LL)                                                                                              \
    do {                                                                                                      \
        if (t->tb.aux)                                                                                        \
            k_rows_sssp<LL, true><<<grid, BLOCK, 0, s>>>(t->bn, blocks, sb0, t->d_srcv, t->d_slots, *t->bG,   \
                                                         t->md, t->st, t->tb);                                \
        else                                                                                                  \
            k_rows_sssp<LL, false><<<grid, BLOCK, 0, s>>>(t->bn, blocks, sb0, t->d_srcv, t->d_slots,          \
                                                          *t->bG, t->md, t->st, t->tb);                       \
    } while (0)
    switch (t->lanes) {
        case 128: ROWS(128); break;
        default: ROWS(64); break;
    }
#undef ROWS
}
#ifndef SPE_SHARED_ROWS_LDS
#define SPE_SHARED_ROWS_LDS 1
#endif
static void launch_rows_shared(spe_table* t, int grid, int32_t blocks, int32_t sb0, hipStream_t s,
                               const int32_t* rsrc, const int2* rli, const double2* rwa, const int2* rng) {
    const Deliv dv{t->d_dlcnt, t->d_dlwork, t->dl_cap};
    if (SPE_SHARED_ROWS_LDS && !t->cx) {   // (contracted targets read three rows: the gather kernel)
        const int64_t work = (int64_t)((blocks + RT_B - 1) / RT_B) * ((t->A + RT_T - 1) / RT_T);
        const int g = (int)std::max<int64_t>(1, std::min<int64_t>(work, 2048));
        if (t->delivery) {   // flags the pendant sources' entries at an ns boundary
            if (t->lanes == 128)
                k_rows_shared_lds<128, true><<<g, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG, t->md,
                                                                 t->st, t->tb, rli, rwa, rng, dv);
            else
                k_rows_shared_lds<64, true><<<g, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG, t->md,
                                                                t->st, t->tb, rli, rwa, rng, dv);
            return;
        }
        if (t->lanes == 128)
            k_rows_shared_lds<128><<<g, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG, t->md, t->st,
                                                       t->tb, rli, rwa, rng);
        else
            k_rows_shared_lds<64><<<g, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG, t->md, t->st,
                                                      t->tb, rli, rwa, rng);
        return;
    }
    if (t->delivery) {
        if (t->lanes == 128)
            k_rows_sssp<128, false, true, true><<<grid, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG,
                                                                        t->md, t->st, t->tb, rli, rwa, dv);
        else
            k_rows_sssp<64, false, true, true><<<grid, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG,
                                                                       t->md, t->st, t->tb, rli, rwa, dv);
        return;
    }
    if (t->lanes == 128)
        k_rows_sssp<128, false, true><<<grid, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG, t->md,
                                                              t->st, t->tb, rli, rwa);
    else
        k_rows_sssp<64, false, true><<<grid, BLOCK, 0, s>>>(t->bn, blocks, sb0, rsrc, t->d_slots, *t->bG, t->md,
                                                             t->st, t->tb, rli, rwa);
}
}  // extern "C++"

int spe_table_build(spe_table* t, void* stream) {
    if (!t) return fail(SPE_EINVAL, "NULL table");
    if (t->multi) {
        const int r = spe::multi_build(t->multi, &t->stats);
        t->built = r == SPE_OK && spe::multi_built(t->multi);
        return r;
    }
    int r = spe_table_build_blocks(t, t->blk0, t->blk1, stream);
    if (r || !t->d_rank || t->md.complete) return r;
    hipStream_t s = stream ? (hipStream_t)stream : t->stream;
    const int64_t items = (int64_t)((t->A + WAVE - 1) / WAVE) * t->A;
    k_owner_replay<<<grid_for(items * WAVE, BLOCK, 8192), BLOCK, 0, s>>>(t->A, t->d_rank, t->d_slot_vertex,
                                                                        t->g->dev, t->md, t->tb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return SPE_OK;
}

static int build_blocks_impl(spe_table* t, int32_t block_begin, int32_t block_end, void* stream);

int spe_table_build_blocks(spe_table* t, int32_t block_begin, int32_t block_end, void* stream) {
    if (!t) return fail(SPE_EINVAL, "NULL table");
    if (t->multi) return fail(SPE_EUNSUPPORTED, "a multi-device table builds whole (spe_table_build)");
    if (block_begin < t->blk0 || block_end > t->blk1 || block_begin > block_end)
        return fail(SPE_EINVAL, "block range not owned by this table");
    const int r = build_blocks_impl(t, block_begin, block_end, stream);
    if (r) return r;
    {   // every record written is visible to host loads of the mapped memory (table_host_reads)
        hipStream_t s = stream ? (hipStream_t)stream : t->stream;
        k_release_system<<<1, 64, 0, s>>>();
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int32_t b = block_begin; b < block_end; ++b) t->blk_built[(size_t)(b - t->blk0)] = 1;
    t->built = std::all_of(t->blk_built.begin(), t->blk_built.end(), [](uint8_t x) { return x != 0; });
    return SPE_OK;
}

int spe_table_build_blocks_into(spe_table* t, int32_t block_begin, int32_t block_end, void* latrel, void* next_hop,
                                void* hops, void* stream) {
    if (!t) return fail(SPE_EINVAL, "NULL table");
    if (t->multi) return fail(SPE_EUNSUPPORTED, "a multi-device table builds whole (spe_table_build)");
    if (block_begin < t->blk0 || block_end > t->blk1 || block_begin > block_end)
        return fail(SPE_EINVAL, "block range not owned by this table");
    if (!latrel || !next_hop || !hops) return fail(SPE_EINVAL, "spe_table_build_blocks_into needs all three fields");
    if (t->tb.prev || t->tb.aux) return fail(SPE_EUNSUPPORTED, "owner-replay / want_aux tables build in place");
    const Table keep = t->tb;
    const int32_t keep_base = t->row_base;
    t->tb.lr = (double2*)latrel;
    t->tb.next = (int32_t*)next_hop;
    t->tb.hops = (uint16_t*)hops;
    t->row_base = block_begin;
    const int r = build_blocks_impl(t, block_begin, block_end, stream);
    t->tb = keep;
    t->row_base = keep_base;
    return r;   // the table's own storage is untouched: nothing is marked built
}

// Shared anchor trees and derived rows (DESIGN §4.1): a batch's relaxation lanes
// are its ROOTS -- each core source, and the anchor of each pruned pendant source,
// once -- and the rows kernel gives every source its root's row (a pendant
// source's with its edge in front).  On a contracted graph a removed source whose
// three neighbours are all roots of the call's range takes no lane (derived, see
// k_rows_derived); any other removed source relaxes on its own lane.  Batches are
// cut at block boundaries into about equal root counts.  Where the weights' sums
// are not exact, k_share_check flags roots whose decisions an offset could change;
// the blocks holding an offset source (pendant or derived) of a flagged root, or a
// source whose derived row failed its own margin (sunsafe), are rebuilt with one
// lane per source.
static int build_shared(spe_table* t, int32_t block_begin, int32_t block_end, hipStream_t s) {
    const spe_graph* g = t->g;
    const spe::HostGraph& h = g->hg;
    const int32_t L = t->lanes;
    const int32_t cap = t->groups * WAVE;   // root lanes one batch's state holds
    const int32_t s_end = std::min(t->A, block_end * WAVE);
    // per slot: root core id (core source, pendant anchor, or a removed source itself),
    // or -3 for a derived source, -1 padding
    // derivable sources (h.cx.der: removed vertices, derived kept ones); their legs
    // h.cx.dlegs[dptr[c] ..) read the lanes of kept vertices `ref` (direct legs: none)
    auto removed = [&](int32_t c) { return t->derive && c >= 0 && h.cx.der[(size_t)c]; };
    auto ndeg = [&](int32_t c) { return h.cx.dptr[(size_t)c + 1] - h.cx.dptr[(size_t)c]; };
    auto nbr = [&](int32_t c, int q) { return h.cx.dlegs[(size_t)h.cx.dptr[(size_t)c] + q].ref; };   // -1: direct
    std::vector<int32_t> tag((size_t)std::max(1, h.nc), -1), lane_of((size_t)std::max(1, h.nc), -1);
    // the call's non-derived roots: a removed source is derivable iff its three neighbours are among them
    int32_t total = 0;
    for (int32_t i = block_begin * WAVE; i < s_end; ++i) {
        const int32_t v = t->attached[(size_t)i];
        const int32_t c0 = h.core_id[(size_t)v];
        const int32_t c = c0 >= 0 ? c0 : h.anchor_core[(size_t)v];
        if (c >= 0 && !removed(c) && tag[(size_t)c] < 0) {
            tag[(size_t)c] = 0;
            ++total;
        }
    }
    // Extra roots (block-range shares of a multi-GPU table: a share holds only its
    // own sources' roots, and the hubs next to its contracted sources sit in other
    // shares).  A neighbour u outside the call's roots becomes a root of its own
    // when it is the ONLY missing neighbour of two or more derivable sources: one
    // lane that saves at least two, so the call never relaxes more lanes than
    // without it.  Repeated while it pays (an added root can leave other sources
    // one neighbour short).  A whole-table build has every neighbour already.
    std::vector<uint8_t> extra((size_t)std::max(1, h.nc), 0);
    if (t->derive) {
        std::vector<int32_t> cand, c1((size_t)std::max(1, h.nc), 0), touched;
        for (int32_t i = block_begin * WAVE; i < s_end; ++i) {
            const int32_t c = h.core_id[(size_t)t->attached[(size_t)i]];
            if (removed(c)) cand.push_back(c);
        }
        auto only_missing = [&](int32_t x) {   // the single non-root leg vertex of x, -1 when 0 or >= 2
            int32_t m = -1, k = 0;
            for (int q = 0; q < ndeg(x); ++q) {
                const int32_t u = nbr(x, q);
                if (u >= 0 && tag[(size_t)u] != 0 && u != m) {
                    m = u;
                    ++k;
                }
            }
            return k == 1 ? m : -1;
        };
        for (int pass = 0; pass < 16; ++pass) {
            for (int32_t u : touched) c1[(size_t)u] = 0;
            touched.clear();
            for (int32_t x : cand) {
                const int32_t u = only_missing(x);
                if (u < 0) continue;
                if (c1[(size_t)u]++ == 0) touched.push_back(u);
            }
            bool added = false;
            for (int32_t u : touched)
                if (c1[(size_t)u] >= 2 && tag[(size_t)u] != 0) {
                    tag[(size_t)u] = 0;
                    extra[(size_t)u] = 1;
                    ++total;
                    added = true;
                }
            if (!added) break;
        }
    }
    std::vector<uint8_t> derivable((size_t)std::max(0, s_end - block_begin * WAVE), 0);
    for (int32_t i = block_begin * WAVE; i < s_end; ++i) {
        const int32_t c = h.core_id[(size_t)t->attached[(size_t)i]];
        if (!removed(c)) continue;
        bool all = true;
        for (int q = 0; q < ndeg(c); ++q) all &= nbr(c, q) < 0 || tag[(size_t)nbr(c, q)] == 0;
        derivable[(size_t)(i - block_begin * WAVE)] = all;
        if (!all) ++total;
    }
    auto root_of = [&](int32_t slot) -> int32_t {
        const int32_t v = t->attached[(size_t)slot];
        const int32_t c0 = h.core_id[(size_t)v];
        if (c0 >= 0 && removed(c0) && derivable[(size_t)(slot - block_begin * WAVE)]) return -3;
        return c0 >= 0 ? c0 : h.anchor_core[(size_t)v];
    };
    const int32_t nb = std::max(1, (total + cap - 1) / cap);
    const int32_t target = (total + nb - 1) / nb;
    std::fill(tag.begin(), tag.end(), -1);
    std::vector<int32_t> roots, deferred;
    std::vector<uint8_t> bad((size_t)std::max(1, h.nc), 0);
    std::vector<uint8_t> dk((size_t)(block_end - block_begin) * WAVE, 0);   // per slot of the batch: derived
    const spe::HostGraph::Share& sh = h.share;
    for (int32_t b = block_begin, bid = 0; b < block_end; ++bid) {
        HIP_TRY(hipStreamSynchronize(s));   // the pinned staging is reused per batch
        roots.clear();
        int32_t e = b;
        auto add = [&](int32_t c) {
            if (c >= 0 && tag[(size_t)c] != bid) {
                tag[(size_t)c] = bid;
                lane_of[(size_t)c] = (int32_t)roots.size();
                roots.push_back(c);
            }
        };
        // The roots of the blocks' other sources first (the cut counts those), then each
        // derivable source of the batch: derived when at most one of its neighbours is
        // not yet a root of the batch (that one becomes a root: no more lanes than the
        // source's own), else on its own lane -- small batches would otherwise re-relax
        // hubs batch after batch.  A batch the second step would overflow is cut before
        // the block that overflows and assembled again (one block always fits: each of
        // its sources costs at most one lane).  Extra roots (above) are added as
        // needed, except in a batch cut back to its first block, where each source
        // again costs at most one lane.
        const int32_t limit = bid + 1 >= nb ? cap : std::min(target, cap);
        int32_t e_max = block_end;
        bool strict = false;
        for (;;) {
            roots.clear();
            e = b;
            while (e < e_max) {
                const size_t before = roots.size();
                for (int32_t l = 0; l < WAVE; ++l) {
                    const int32_t slot = e * WAVE + l;
                    if (slot >= t->A) break;
                    const int32_t c = root_of(slot);
                    if (c != -3) add(c);
                }
                // this block starts the next batch (the last planned batch takes the rest up to `cap`)
                if (e > b && (int32_t)roots.size() > limit) {
                    for (size_t i = before; i < roots.size(); ++i) tag[(size_t)roots[i]] = -1;
                    roots.resize(before);
                    break;
                }
                ++e;
            }
            std::fill(dk.begin(), dk.begin() + (size_t)(e - b) * WAVE, 0);
            int32_t over = -1;
            for (int32_t i = 0; i < (e - b) * WAVE && over < 0; ++i) {
                const int32_t slot = b * WAVE + i;
                if (slot >= t->A || root_of(slot) != -3) continue;
                const int32_t x = h.core_id[(size_t)t->attached[(size_t)slot]];
                int32_t miss = 0, plain = 0;   // (plain: missing leg vertices that are not extra roots)
                for (int q = 0; q < ndeg(x); ++q) {
                    const int32_t u = nbr(x, q);
                    if (u < 0) continue;
                    bool dup = false;   // (two legs may read one lane)
                    for (int p = 0; p < q; ++p) dup |= nbr(x, p) == u;
                    if (dup) continue;
                    miss += tag[(size_t)u] != bid;
                    plain += tag[(size_t)u] != bid && !extra[(size_t)u];
                }
                // (several batches: an extra root would be relaxed again in each, so there
                // every source costs at most one lane, as in a batch cut back to one block)
                const bool derive_it = (strict || nb > 1) ? miss <= 1 : plain <= 1;
                if ((int32_t)roots.size() + (derive_it ? miss : 1) > cap) {
                    over = b + i / WAVE;
                    break;
                }
                if (derive_it) {
                    for (int q = 0; q < ndeg(x); ++q) add(nbr(x, q));   // (add skips -1)
                    dk[(size_t)i] = 1;
                } else {
                    add(x);
                }
            }
            if (over < 0) break;
            for (int32_t c : roots) tag[(size_t)c] = -1;
            strict = over <= b;
            e_max = std::max(b + 1, over);
        }
        const int32_t R = (int32_t)roots.size();
        if (R > cap) return fail(SPE_ESTATE, "shared batch exceeds the state (one block's roots > groups * 64)");
        const int32_t nblk = e - b;
        // relaxation lanes: the roots (core sources of the batch engine's state)
        const int32_t bpg = std::max(1, L / WAVE);
        const int32_t rb = std::max(1, (R + WAVE - 1) / WAVE);
        const int32_t pb = (rb + bpg - 1) / bpg * bpg;
        for (int32_t i = 0; i < pb * WAVE; ++i) {
            const int32_t c = i < R ? roots[(size_t)i] : -1;
            t->h_srcv[i] = c < 0 ? -1 : h.corev[(size_t)c];
            int32_t cc = c;
            if (t->cx && c >= 0) cc = h.cx.kid[(size_t)c] >= 0 ? h.cx.kid[(size_t)c] : -2;
            t->h_srcv[pb * WAVE + i] = cc;
        }
        // rows: every source slot of blocks [b, e), its root's lane and pendant prefix,
        // or (derived) its record of neighbour lanes
        const size_t ns = (size_t)nblk * WAVE;
        double2* hw = reinterpret_cast<double2*>(t->h_rows);
        int2* hl = reinterpret_cast<int2*>(hw + ns);
        int32_t* hr = reinterpret_cast<int32_t*>(hl + ns);
        int32_t nder = 0;
        size_t nlegs = 0;   // derive: every source slot's legs (k_rows_derived)
        for (int32_t i = 0; i < nblk * WAVE; ++i) {
            const int32_t slot = b * WAVE + i;
            int32_t c = slot < t->A ? root_of(slot) : -1;
            if (c == -3 && !dk[(size_t)i]) c = h.core_id[(size_t)t->attached[(size_t)slot]];   // on its own lane
            const int32_t v = (slot < t->A && c != -1) ? t->attached[(size_t)slot] : -1;
            hr[i] = v;
            hw[i] = make_double2(0.0, 1.0);
            if (c == -3) {   // derived: its legs' lanes
                const int32_t x = h.core_id[(size_t)v];
                const int32_t l0 = (int32_t)nlegs;
                for (int q = 0; q < ndeg(x); ++q) {
                    const spe::HostGraph::Contracted::Leg& gl = h.cx.dlegs[(size_t)h.cx.dptr[(size_t)x] + q];
                    DLeg d{};
                    d.w = gl.w;
                    d.a = gl.a;
                    d.ref = gl.ref >= 0 ? lane_of[(size_t)gl.ref] : leg_direct_ref(gl.tc);
                    d.hopinc = gl.hop | (gl.inc << 29);
                    t->h_der[nlegs++] = d;
                }
                hl[i] = make_int2(l0, ndeg(x) | (1 << 16));
                ++nder;
                continue;
            }
            hl[i] = make_int2(c >= 0 ? lane_of[(size_t)c] : -1, -1);
            if (v >= 0 && h.core_id[(size_t)v] < 0) {   // pendant: the edge s -> anchor in front
                const int32_t kx = h.fiptr[(size_t)v];
                const double fs = h.vfac[(size_t)v];
                hl[i].y = h.corev[(size_t)h.anchor_core[(size_t)v]];
                hw[i] = make_double2(h.fiw[(size_t)kx], (std::isnan(fs) ? 1.0 : 1.0 * fs) * h.fia[(size_t)kx]);
            }
            if (t->derive) {   // one leg: the root's lane, behind the pendant edge for a pendant source
                DLeg d{};
                d.w = hw[i].x;
                d.a = hw[i].y;
                d.ref = hl[i].x;
                d.hopinc = hl[i].y >= 0 ? (hl[i].y | (1 << 29)) : -1;
                const int32_t l0 = (int32_t)nlegs;
                if (v >= 0) t->h_der[nlegs++] = d;
                hl[i] = make_int2(l0, (v >= 0 ? 1 : 0) | (d.hopinc >= 0 ? 1 << 16 : 0));
            }
        }
        // per tile of RT_B blocks: the span of root lanes its sources read (k_rows_shared_lds)
        const int32_t ntile = (nblk + RT_B - 1) / RT_B;
        int2* hg = reinterpret_cast<int2*>(hr + ns);
        for (int32_t k = 0; k < ntile; ++k) {
            int32_t lo = INT32_MAX, hi = -1;
            for (int32_t i = k * RT_B * WAVE; i < std::min(nblk, (k + 1) * RT_B) * WAVE; ++i)
                if (hl[i].x >= 0) {
                    lo = std::min(lo, hl[i].x);
                    hi = std::max(hi, hl[i].x);
                }
            hg[k] = hi >= 0 ? make_int2(lo, hi) : make_int2(0, -1);
        }
        int32_t* d_rsrc = t->rsrc_buf[0];
        int2* d_rli = t->rli_buf[0];
        double2* d_rwa = t->rwa_buf[0];
        int2* d_rng = t->rng_buf[0];
        HIP_TRY(hipMemcpyAsync(t->d_srcv, t->h_srcv, sizeof(int32_t) * pb * WAVE, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->d_srcc, t->h_srcv + pb * WAVE, sizeof(int32_t) * pb * WAVE, hipMemcpyHostToDevice,
                               s));
        HIP_TRY(hipMemcpyAsync(d_rsrc, hr, sizeof(int32_t) * ns, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rli, hl, sizeof(int2) * ns, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rwa, hw, sizeof(double2) * ns, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rng, hg, sizeof(int2) * ntile, hipMemcpyHostToDevice, s));
        if (t->derive && nlegs > 0)
            HIP_TRY(hipMemcpyAsync(t->d_der, t->h_der, sizeof(DLeg) * nlegs, hipMemcpyHostToDevice, s));
        // the margin proof rides on the relaxation where it can (k_relax_s + 128-lane heavy passes)
        t->mg_track = !sh.exact && t->tight != nullptr && L == 128 && t->relax_kernel == SPE_RELAX_LDS_RING &&
                      t->delta <= 0.0;
        // 1 / wmin rounded up (margin_near: never a smaller margin than k_share_check's)
        t->mg_invw = sh.wmin > 0.0 ? std::nextafter(1.0 / sh.wmin, INFINITY) : INFINITY;
        t->mg_omax = sh.omax;
        t->mg_hmax = (double)h.n + 2.0;
        int r = relax_to_convergence(t, rb, s);
        const bool tracked = t->mg_track;
        t->mg_track = false;
        if (r) return r;
        t->stats.relaxed_lanes += R;
        t->stats.derived_sources += nder;
        bool any_bad = false;
        if (!sh.exact) {
            const int32_t groups = L > WAVE ? pb / bpg : pb * (WAVE / L);
            HIP_TRY(hipMemsetAsync(t->d_unsafe, 0, (size_t)groups * L, s));
            if (tracked) {
                LaunchTimer lt(t, s, SPE_K_HEAVY);
                k_tight_reduce<<<groups, BLOCK, 0, s>>>(t->bn, t->tight, t->d_unsafe);
            } else {
                LaunchTimer lt(t, s, SPE_K_HEAVY);   // (accounted with the heavy-vertex passes)
                const int grid = grid_for((int64_t)groups * (t->bn + t->bhp->nseg) * WAVE, BLOCK, 8192);
                const double hmax = (double)h.n + 2.0;
                if (L == 128)
                    k_share_check<128><<<grid, BLOCK, 0, s>>>(groups, t->bn, t->d_srcv, *t->bG, t->st, *t->bhp,
                                                              sh.wmin, sh.omax, hmax, t->d_unsafe);
                else
                    k_share_check<64><<<grid, BLOCK, 0, s>>>(groups, t->bn, t->d_srcv, *t->bG, t->st, *t->bhp,
                                                             sh.wmin, sh.omax, hmax, t->d_unsafe);
            }
            HIP_TRY(hipMemcpyAsync(t->h_unsafe, t->d_unsafe, (size_t)R, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (int32_t i = 0; i < R; ++i)
                if (t->h_unsafe[i]) {
                    bad[(size_t)roots[(size_t)i]] = 1;
                    any_bad = true;
                }
        }
        const int32_t sb0 = b - t->row_base;
        const Deliv dv{t->d_dlcnt, t->d_dlwork, t->dl_cap};
        if (t->delivery) {
            HIP_TRY(hipMemsetAsync(t->d_dlcnt, 0, sizeof(uint32_t) * 2 * (size_t)nblk, s));
        }
        {
            LaunchTimer lt(t, s, SPE_K_ROWS);
            if (t->derive) {
                HIP_TRY(hipMemsetAsync(t->d_sunsafe, 0, ns, s));
                const double hmax = (double)h.n + 2.0;
                if (t->nr > 0 && !(SPE_ROWS_LM && SPE_LM_FUSE)) {
                    const int32_t groups = pb / bpg;   // (L = 128: contracted tables)
                    const int grid = grid_for((int64_t)groups * t->nr * WAVE, BLOCK, 8192);
                    k_expand_removed<128><<<grid, BLOCK, 0, s>>>(groups, t->bn, t->nr, *t->bG, t->st, t->d_dx,
                                                                 t->d_rtx, t->d_rorig, sh.exact ? 0 : 1, sh.wmin,
                                                                 sh.omax, hmax);
                }
                const int64_t ntt = (t->A + SPE_DERIVED_TT - 1) / SPE_DERIVED_TT;
                const int64_t items = (ntt + SPE_DERIVED_TC - 1) / SPE_DERIVED_TC * nblk;
                const int grid = (grid_for(items * WAVE, BLOCK, 8192) + 7) & ~7;
#ifndef SPE_ROWS_LEAN
#define SPE_ROWS_LEAN 1   // 0: always the general kernel (A/B)
#endif
                if (SPE_ROWS_LM) {   // lane-major: stage the root lanes per target slot, then rows
                    const int32_t groups = pb / bpg;
                    const int64_t sitems = (int64_t)groups * ((t->A + LM_TS - 1) / LM_TS);
                    k_stage_lanes<<<(int)std::min<int64_t>(sitems, 8192), BLOCK, 0, s>>>(
                        groups, t->bn, t->nr, t->A, t->d_slots, t->st.D, t->st.RT, t->d_dx, t->d_rtx, t->d_xd,
                        t->d_xrt, *t->bG, t->d_rorig, sh.exact ? 0 : 1, sh.wmin, sh.omax, hmax);
                    const int64_t ritems = (int64_t)nblk * ((t->A + LM_T - 1) / LM_T);
                    const int rgrid = (int)((std::min<int64_t>(ritems, 8192) + 7) & ~(int64_t)7);
                    if (t->delivery) {   // the same rows, entries at an ns boundary flagged for the re-fold
                        if (t->pend_targets)
                            k_rows_lm<true, true><<<rgrid, BLOCK, 0, s>>>(nblk, sb0, d_rsrc, t->d_slots, *t->bG, t->md,
                                                                          t->tb, d_rli, t->d_der, t->d_xd, t->d_xrt,
                                                                          sh.wmin, sh.omax, hmax, sh.exact ? 1 : 0,
                                                                          t->d_sunsafe, dv);
                        else
                            k_rows_lm<false, true><<<rgrid, BLOCK, 0, s>>>(nblk, sb0, d_rsrc, t->d_slots, *t->bG, t->md,
                                                                           t->tb, d_rli, t->d_der, t->d_xd, t->d_xrt,
                                                                           sh.wmin, sh.omax, hmax, sh.exact ? 1 : 0,
                                                                           t->d_sunsafe, dv);
                        if (!t->pend_targets)
                            k_rows_self<<<(nblk * WAVE + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(nblk, sb0, b * WAVE, d_rsrc,
                                                                                           *t->bG, t->md, t->tb);
                    } else if (t->pend_targets) {
                        k_rows_lm<true><<<rgrid, BLOCK, 0, s>>>(nblk, sb0, d_rsrc, t->d_slots, *t->bG, t->md, t->tb,
                                                                d_rli, t->d_der, t->d_xd, t->d_xrt, sh.wmin, sh.omax,
                                                                hmax, sh.exact ? 1 : 0, t->d_sunsafe);
                    } else {
                        k_rows_lm<false><<<rgrid, BLOCK, 0, s>>>(nblk, sb0, d_rsrc, t->d_slots, *t->bG, t->md, t->tb,
                                                                 d_rli, t->d_der, t->d_xd, t->d_xrt, sh.wmin, sh.omax,
                                                                 hmax, sh.exact ? 1 : 0, t->d_sunsafe);
                        k_rows_self<<<(nblk * WAVE + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(nblk, sb0, b * WAVE, d_rsrc,
                                                                                       *t->bG, t->md, t->tb);
                    }
                } else if (t->pend_targets || !SPE_ROWS_LEAN) {   // the general kernel: pendant targets and self entries inline
                    k_rows_derived<128, SPE_DERIVED_TT><<<grid, BLOCK, 0, s>>>(
                        t->bn, nblk, sb0, d_rsrc, t->d_slots, *t->bG, t->md, t->st.D, t->st.RT, t->tb, d_rli,
                        t->d_der, t->d_dx, t->d_rtx, t->nr, sh.wmin, sh.omax, hmax, sh.exact ? 1 : 0, t->d_sunsafe);
                } else {   // lean kernel (4 waves / SIMD), then the self entries
                    k_rows_derived<128, SPE_DERIVED_TT, SPE_DERIVED_TC, false><<<grid, BLOCK, 0, s>>>(
                        t->bn, nblk, sb0, d_rsrc, t->d_slots, *t->bG, t->md, t->st.D, t->st.RT, t->tb, d_rli,
                        t->d_der, t->d_dx, t->d_rtx, t->nr, sh.wmin, sh.omax, hmax, sh.exact ? 1 : 0, t->d_sunsafe);
                    k_rows_self<<<(nblk * WAVE + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(nblk, sb0, b * WAVE, d_rsrc,
                                                                                   *t->bG, t->md, t->tb);
                }
            } else {
                launch_rows_shared(t, grid_for((int64_t)nblk * t->A * WAVE, BLOCK, 8192), nblk, sb0, s, d_rsrc,
                                   d_rli, d_rwa, d_rng);
            }
            if (t->delivery) {
                // the re-fold walks this batch's state: after its rows, before the next batch's
                // relaxation (same stream) and before the direct-edge overlay
                HIP_TRY(hipEventRecord(t->ev_dl[0], s));
                const int rgrid = grid_for((int64_t)nblk * t->dl_cap, BLOCK, 2048);
                if (L == 128)
                    k_refold_delivery<128><<<rgrid, BLOCK, 0, s>>>(t->bn, nblk, sb0, t->d_slots, *t->bG, t->st, t->tb,
                                                                   t->d_der, d_rwa, dv, t->d_dlcnt + nblk);
                else
                    k_refold_delivery<64><<<rgrid, BLOCK, 0, s>>>(t->bn, nblk, sb0, t->d_slots, *t->bG, t->st, t->tb,
                                                                  t->d_der, d_rwa, dv, t->d_dlcnt + nblk);
                HIP_TRY(hipEventRecord(t->ev_dl[1], s));
            }
        }
        if (t->md.prefer) {
            LaunchTimer lt(t, s, SPE_K_DIRECT);
            k_direct_overlay<<<(nblk * WAVE + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(nblk, sb0, d_rsrc, t->d_vertex_slot,
                                                                                 g->dev, t->tb);
        }
        HIP_TRY(hipGetLastError());
        bool any_sunsafe = false;
        const size_t deferred0 = deferred.size();
        if (t->delivery)
            HIP_TRY(hipMemcpyAsync(t->h_dl, t->d_dlcnt, sizeof(uint32_t) * 2 * (size_t)nblk, hipMemcpyDeviceToHost, s));
        if (t->derive) {
            HIP_TRY(hipMemcpyAsync(t->h_sunsafe, t->d_sunsafe, ns, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (size_t i = 0; i < ns && !any_sunsafe; ++i) any_sunsafe = t->h_sunsafe[i] != 0;
        }
        if (any_bad || any_sunsafe)
            for (int32_t blk = b; blk < e; ++blk)
                for (int32_t l = 0; l < WAVE; ++l) {
                    const int32_t slot = blk * WAVE + l;
                    if (slot >= t->A) break;
                    const size_t i = (size_t)(slot - b * WAVE);
                    bool d = any_sunsafe && t->h_sunsafe[i];
                    const int32_t v = t->attached[(size_t)slot];
                    int32_t c = root_of(slot);
                    if (c == -3 && !dk[i]) c = h.core_id[(size_t)v];
                    if (!d && any_bad) {
                        // an offset source of a flagged root (a core source is its own root: exact)
                        if (c == -3) {
                            const int32_t x = h.core_id[(size_t)v];
                            for (int q = 0; q < ndeg(x); ++q) d |= nbr(x, q) >= 0 && bad[(size_t)nbr(x, q)] != 0;
                        } else if (c >= 0 && h.core_id[(size_t)v] != c) {
                            d = bad[(size_t)c] != 0;
                        }
                    }
                    if (d) {
                        deferred.push_back(blk);
                        break;
                    }
                }
        if (t->delivery) {
            // flagged entries count in full; a block over its cap joins the blocks rebuilt one lane
            // per source; changes count where the re-fold is what the block keeps
            HIP_TRY(hipStreamSynchronize(s));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, t->ev_dl[0], t->ev_dl[1]));
            t->stats.delivery_seconds += 1e-3 * (double)ms;
            std::vector<uint8_t> rebuilt((size_t)nblk, 0);
            for (size_t i = deferred0; i < deferred.size(); ++i) rebuilt[(size_t)(deferred[i] - b)] = 1;
            for (int32_t k = 0; k < nblk; ++k) {
                t->stats.delivery_flagged += t->h_dl[k];
                if (t->h_dl[k] > (uint32_t)t->dl_cap) {
                    t->stats.delivery_fallback = 2;
                    if (!rebuilt[(size_t)k]) deferred.push_back(b + k);
                } else if (!rebuilt[(size_t)k]) {
                    t->stats.delivery_changed += t->h_dl[nblk + k];
                }
            }
        }
        if (t->prof) {
            HIP_TRY(hipStreamSynchronize(s));
            r = resolve_profile(t, true);
            if (r) return r;
        }
        b = e;
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (!deferred.empty()) {   // one lane per source for the flagged blocks
        std::sort(deferred.begin(), deferred.end());
        deferred.erase(std::unique(deferred.begin(), deferred.end()), deferred.end());
        spe_build_stats keep = t->stats;
        t->share_off = true;
        int r = SPE_OK;
        for (size_t i = 0; i < deferred.size() && !r;) {
            size_t j = i + 1;
            while (j < deferred.size() && deferred[j] == deferred[j - 1] + 1) ++j;
            r = build_blocks_impl(t, deferred[i], deferred[j - 1] + 1, s);
            keep.iterations += t->stats.iterations;
            keep.active_rounds += t->stats.active_rounds;
            keep.launches += t->stats.launches;
            keep.relaxed_lanes += t->stats.relaxed_lanes;
            keep.fallback_blocks += deferred[j - 1] + 1 - deferred[i];
            i = j;
        }
        t->share_off = false;
        t->stats = keep;
        if (r) return r;
    }
    return SPE_OK;
}

static int build_blocks_impl(spe_table* t, int32_t block_begin, int32_t block_end, void* stream) {
    HIP_TRY(hipSetDevice(t->g->device));
    if (t->trace)   // where the relaxation state lives (run-to-run placement studies)
        for (int i = 0; i < 2; ++i)
            fprintf(stderr, "spe-trace-buf %d D %p P %p RT %p in %p mark %p\n", i, (void*)t->st_buf[i].D,
                    (void*)t->st_buf[i].P, (void*)t->st_buf[i].RT, (void*)t->inflag[i], (void*)t->mark[i]);
    hipStream_t s = stream ? (hipStream_t)stream : t->stream;
    const auto t0 = std::chrono::steady_clock::now();
    const spe_graph* g = t->g;
    t->stats = spe_build_stats{};
    t->stats.replica_mismatches = -1;   // one device: nothing to verify
    t->stats.delivery_fallback = t->dl_fallback;
    const bool ovl = t->overlap && !t->md.complete && t->engine == SPE_ENGINE_BATCH;
    hipStream_t rs = ovl ? t->rows_stream : s;
    if (t->share && !t->share_off) {
        // one stream: the rows kernel's grid holds every CU slot while it runs, so a
        // concurrent relaxation of the next batch only queues behind it (the launches
        // between them wait for slots); one batch of every root, then its rows, was
        // as fast or faster (C4 0.1275 vs 0.130 s, same box, two passes)
        const int r = build_shared(t, block_begin, block_end, s);
        if (r) return r;
        t->stats.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        t->stats.n_devices = 1;
        return SPE_OK;
    }
    int buf = 0;
    for (int32_t b = block_begin; b < block_end; b += t->groups) {
        const int32_t groups = std::min(t->groups, block_end - b);
        HIP_TRY(hipStreamSynchronize(s));   // h_srcv is reused per batch
        if (ovl) {   // this batch's buffers: free once the rows two batches back are written
            t->st = t->st_buf[buf];
            t->d_srcv = t->srcv_buf[buf];
            t->d_srcc = t->srcc_buf[buf];
            if (t->rows_pending[buf]) HIP_TRY(hipStreamWaitEvent(s, t->ev_rows[buf], 0));
        }
        // blocks of source entries: a lane group of L > 64 spans L / 64 blocks, so
        // an odd tail is padded with empty (-1) blocks
        const int32_t bpg = std::max(1, t->lanes / WAVE);
        const int32_t pb = (groups + bpg - 1) / bpg * bpg;
        for (int32_t gi = 0; gi < pb; ++gi)
            for (int32_t l = 0; l < WAVE; ++l) {
                const int32_t slot = (b + gi) * WAVE + l;
                const int32_t v = (gi < groups && slot < t->A) ? t->attached[slot] : -1;
                t->h_srcv[gi * WAVE + l] = v;
                int32_t c = v < 0 ? -1 : (g->hg.core_id[v] >= 0 ? g->hg.core_id[v] : -2);
                if (t->cx && c >= 0) c = g->hg.cx.kid[c] >= 0 ? g->hg.cx.kid[c] : -2;   // (a contracted source: -2)
                t->h_srcv[(pb + gi) * WAVE + l] = c;
            }
        HIP_TRY(hipMemcpyAsync(t->d_srcv, t->h_srcv, sizeof(int32_t) * pb * WAVE, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->d_srcc, t->h_srcv + pb * WAVE, sizeof(int32_t) * pb * WAVE,
                               hipMemcpyHostToDevice, s));
        const int32_t sb0 = b - t->row_base;
        const int64_t items = (int64_t)groups * t->A;
        const int row_grid = grid_for(items * WAVE, BLOCK, 8192);
        if (t->md.complete) {
            LaunchTimer lt(t, s, SPE_K_DIRECT);
            k_rows_direct<<<row_grid, BLOCK, 0, s>>>(groups, sb0, t->d_srcv, t->d_slot_vertex, g->dev, t->md, t->tb);
        } else if (t->engine == SPE_ENGINE_LDS) {
            {
                LaunchTimer lt(t, s, SPE_K_LDS);
                const int32_t s0 = b * WAVE, s1 = std::min(t->A, (b + groups) * WAVE);
                const size_t bytes = lds_bytes(g->hg.nc);
                int grid = std::min(s1 - s0, t->lds_grid);
                if (grid >= 8) grid -= grid % 8;   // whole XCD rounds (see k_sssp_lds's slot order)
                if (t->lds_debug && !t->d_lds_dbg) {
                    if (int r = dev_alloc(t->allocs, &t->d_lds_dbg, 16)) return r;
                    HIP_TRY(hipMemset(t->d_lds_dbg, 0, 16 * sizeof(unsigned long long)));
                }
                k_sssp_lds<<<std::max(1, grid), LDS_T, bytes, s>>>(s0, s1, t->d_slots, t->row_base, g->dev, t->md, t->tb,
                                                                   t->lsc, t->d_lds_dbg);
                if (t->d_lds_dbg) {
                    unsigned long long h[16];
                    HIP_TRY(hipStreamSynchronize(s));
                    HIP_TRY(hipMemcpy(h, t->d_lds_dbg, sizeof(h), hipMemcpyDeviceToHost));
                    const double nsrc = (double)std::max(1ull, h[10]);
                    fprintf(stderr, "spe-lds sources %llu rounds/src %.1f levels/src %.1f us/src: init %.1f push %.1f "
                            "parent %.1f lat %.1f tree-build %.1f tree-pass %.1f rows %.1f | push: wave0 flush %.1f barrier %.1f\n", h[10], h[8] / nsrc, h[9] / nsrc,
                            h[0] / nsrc / 100.0, h[1] / nsrc / 100.0, h[2] / nsrc / 100.0, h[3] / nsrc / 100.0,
                            h[4] / nsrc / 100.0, h[5] / nsrc / 100.0, h[6] / nsrc / 100.0, h[11] / nsrc / 100.0,
                            h[12] / nsrc / 100.0);
                }
            }
            if (t->md.prefer) {
                LaunchTimer lt(t, s, SPE_K_DIRECT);
                k_direct_overlay<<<(groups * WAVE + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(
                    groups, sb0, t->d_srcv, t->d_vertex_slot, g->dev, t->tb);
            }
        } else if (t->engine == SPE_ENGINE_FW) {
            if (!t->fw_done) {
                LaunchTimer lt(t, s, SPE_K_FW);
                if (int r = fw3_closure(g, t->fw, t->fw_ld, s)) return r;
                t->fw_done = true;
            }
            {
                LaunchTimer lt(t, s, SPE_K_FW);
                k_fw_state<<<dim3((g->hg.nc + WAVE - 1) / WAVE, groups), BLOCK, 0, s>>>(
                    g->hg.nc, t->fw_ld, t->d_srcv, t->d_srcc, g->dev, t->fw, t->st);
            }
            {
                LaunchTimer lt(t, s, SPE_K_ROWS);
                launch_rows_sssp(t, row_grid, groups, sb0, s);
            }
            if (t->md.prefer) {
                LaunchTimer lt(t, s, SPE_K_DIRECT);
                k_direct_overlay<<<(groups * WAVE + BLOCK - 1) / BLOCK, BLOCK, 0, s>>>(
                    groups, sb0, t->d_srcv, t->d_vertex_slot, g->dev, t->tb);
            }
        } else {
            int r = relax_to_convergence(t, groups, s);
            if (r) return r;
            t->stats.relaxed_lanes += std::max(0, std::min(t->A, (b + groups) * WAVE) - b * WAVE);
            if (ovl) {
                HIP_TRY(hipEventRecord(t->ev_relaxed, s));
                HIP_TRY(hipStreamWaitEvent(rs, t->ev_relaxed, 0));
            }
            {
                LaunchTimer lt(t, rs, SPE_K_ROWS);
                launch_rows_sssp(t, row_grid, groups, sb0, rs);
            }
            if (t->md.prefer) {
                LaunchTimer lt(t, rs, SPE_K_DIRECT);
                k_direct_overlay<<<(groups * WAVE + BLOCK - 1) / BLOCK, BLOCK, 0, rs>>>(
                    groups, sb0, t->d_srcv, t->d_vertex_slot, g->dev, t->tb);
            }
            if (ovl) {
                HIP_TRY(hipEventRecord(t->ev_rows[buf], rs));
                t->rows_pending[buf] = true;
                buf ^= 1;
            }
        }
        HIP_TRY(hipGetLastError());
        if (t->prof) {
            HIP_TRY(hipStreamSynchronize(s));
            int r = resolve_profile(t, !ovl);
            if (r) return r;
        }
    }
    if (ovl) {
        HIP_TRY(hipStreamSynchronize(rs));
        t->rows_pending[0] = t->rows_pending[1] = false;
        t->st = t->st_buf[0];
        t->d_srcv = t->srcv_buf[0];
        t->d_srcc = t->srcc_buf[0];
        if (t->prof) {
            int r = resolve_profile(t);
            if (r) return r;
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    t->stats.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    t->stats.n_devices = 1;
    return SPE_OK;
}

int spe_table_profile_enable(spe_table* t, int32_t enable) {
    if (!t) return fail(SPE_EINVAL, "NULL table");
    if (t->multi) return spe::multi_profile_enable(t->multi, enable);
    t->prof = enable != 0;
    t->kp = spe_kernel_profile{};
    t->pending.clear();
    t->ev_next = 0;
    return SPE_OK;
}

int spe_table_profile_get(const spe_table* t, spe_kernel_profile* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return spe::multi_profile_get(t->multi, out);
    *out = t->kp;
    return SPE_OK;
}

int spe_table_build_stats(const spe_table* t, spe_build_stats* out) {
    if (out && out->struct_size != sizeof(spe_build_stats)) return fail(SPE_EINVAL, ABI_MSG("spe_build_stats"));
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    *out = t->stats;
    out->struct_size = sizeof(spe_build_stats);
    return SPE_OK;
}

int spe_table_layout_get(const spe_table* t, spe_table_layout* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (out->struct_size != sizeof(spe_table_layout)) return fail(SPE_EINVAL, ABI_MSG("spe_table_layout"));
    if (t->multi) return spe::multi_layout(t->multi, out);
    out->n_devices = 1;
    out->device = t->g->device;
    out->n_attached = t->A;
    out->block_begin = t->blk0;
    out->block_end = t->blk1;
    out->elems = (int64_t)(t->blk1 - t->blk0) * t->A * WAVE;
    out->latrel = t->tb.lr;
    out->next_hop = t->tb.next;
    out->hops = t->tb.hops;
    out->groups_per_launch = t->groups;
    out->engine = t->engine;
    out->lanes_per_group = t->lanes;
    out->relax_kernel = t->relax_kernel;
    out->contracted_vertices = t->cx ? t->bn : 0;
    out->shared_sources = t->share ? 1 : 0;
    out->host_reads = t->host_rd.load(std::memory_order_acquire);
    out->host_prefault = t->pf_state.load(std::memory_order_acquire);
    const int64_t now = std::chrono::duration_cast<std::chrono::nanoseconds>(
                            std::chrono::steady_clock::now().time_since_epoch()).count();
    out->host_prefault_s = 1e-9 * (double)(out->host_prefault == 2 ? t->pf_ns.load(std::memory_order_acquire)
                                           : out->host_prefault == 1 ? now - t->pf_t0.load() : 0);
    return SPE_OK;
}

}  // extern "C"

// Staging of the host-side lookups (caller holds h->mu): two streams on `device`
// and two slots of room for `q` queries each (0: only the single-entry buffer).
static int host_lookup_reserve(spe_table::HostLookup* h, int32_t device, int64_t q) {
    if (h->device < 0) {
        HIP_TRY(hipSetDevice(device));
        for (int k = 0; k < 2; ++k) HIP_TRY(hipStreamCreateWithFlags(&h->sstream[k], hipStreamNonBlocking));
        h->stream = h->sstream[0];
        HIP_TRY(hipHostMalloc((void**)&h->h_entry, 64, hipHostMallocDefault));
        h->device = device;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (q <= h->cap) return SPE_OK;
    for (int k = 0; k < 2; ++k) {
        for (void* p : {(void*)h->d_pairs[k], (void*)h->d_lat[k], (void*)h->d_rel[k], (void*)h->d_ok[k]})
            if (p) HIP_TRY(hipFree(p));
        for (void* p : {(void*)h->h_pairs[k], (void*)h->h_lat[k], (void*)h->h_rel[k], (void*)h->h_ok[k]})
            if (p) HIP_TRY(hipHostFree(p));
        h->d_pairs[k] = nullptr;
        h->d_lat[k] = h->d_rel[k] = nullptr;
        h->d_ok[k] = nullptr;
        h->h_pairs[k] = nullptr;
        h->h_lat[k] = h->h_rel[k] = nullptr;
        h->h_ok[k] = nullptr;
    }
    h->cap = 0;
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipMalloc(&h->d_pairs[k], (size_t)q * sizeof(int2)));
        HIP_TRY(hipMalloc(&h->d_lat[k], (size_t)q * sizeof(double)));
        HIP_TRY(hipMalloc(&h->d_rel[k], (size_t)q * sizeof(double)));
        HIP_TRY(hipMalloc(&h->d_ok[k], (size_t)q));
        HIP_TRY(hipHostMalloc((void**)&h->h_pairs[k], (size_t)q * sizeof(int2), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void**)&h->h_lat[k], (size_t)q * sizeof(double), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void**)&h->h_rel[k], (size_t)q * sizeof(double), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void**)&h->h_ok[k], (size_t)q, hipHostMallocDefault));
    }
    h->cap = q;
    return SPE_OK;
}

// memcpy on up to 8 threads (host <-> pinned staging: one thread moves ~10 GB/s)
static void pcopy(void* dst, const void* src, size_t bytes) {
    const size_t per = (size_t)4 << 20;
    const int nt = (int)std::min<size_t>(8, std::max<size_t>(1, bytes / per));
    if (nt <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> th;
    for (int k = 1; k < nt; ++k)
        th.emplace_back([=] {
            const size_t a = bytes * k / nt, b = bytes * (k + 1) / nt;
            std::memcpy((char*)dst + a, (const char*)src + a, b - a);
        });
    std::memcpy(dst, src, bytes / nt);
    for (auto& x : th) x.join();
}

