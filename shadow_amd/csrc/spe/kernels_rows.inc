// kernels_rows.inc -- part of spe.hip (one translation unit; included inside its
// anonymous namespace).  Row kernels: state -> table rows (k_rows_sssp, shared / derived rows, the
// expansion of removed vertices, the offset margin check, DIRECT rows).

// (s, s) entry: DIRECT self-loop, the row's [s] path, or the SELF rule.
__device__ __forceinline__ void self_entry(const DevGraph& G, const RowMode& md, int32_t s, double& L_,
                                           double& R, int32_t& N, int32_t& H) {
    const double fs = G.vfac[s];
    const double lw = G.loop_w[s];
    const bool loop = has_attr(lw);
    if (md.complete && !loop) return;                    // get_eid(s, s) fails: unroutable
    if ((md.complete || md.prefer) && loop) {            // _topology_lookupDirectPath(s, s)
        double r = 1.0;
        if (has_attr(fs)) r *= fs;
        if (has_attr(fs)) r *= fs;
        r *= G.loop_a[s];
        L_ = 0.0 + lw;
        R = r;
        N = s;
        H = 1;
    } else if (md.self_mode == SPE_SELF_ROW && loop) {   // path [s], shd-topology.c:1456-1484
        double r = 1.0;
        if (has_attr(fs)) r *= fs;
        r *= G.loop_a[s];
        double l = 0.0 + lw;
        if (l == 0) l = 1;
        L_ = l;
        R = r;
        N = s;
        H = 1;
    } else if (G.self_other[s] >= 0) {                   // SELF rule
        L_ = G.self_w2[s];
        R = G.self_a2[s];
        N = G.self_other[s];
        H = 2;
    }
}

// DIRECT (s, t != s): first edge s->t in the out-CSR (merged, get_eid's edge).
__device__ __forceinline__ bool direct_entry(const DevGraph& G, int32_t s, int32_t t, double& L_, double& R,
                                             int32_t& N, int32_t& H) {
    int32_t lo = G.dptr[s], hi = G.dptr[s + 1];
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (G.dcol[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= G.dptr[s + 1] || G.dcol[lo] != t) return false;
    const double fs = G.vfac[s], ft = G.vfac[t];
    double r = 1.0;
    if (has_attr(fs)) r *= fs;
    if (has_attr(ft)) r *= ft;
    r *= G.darep[lo];
    L_ = 0.0 + G.dwrep[lo];
    R = r;
    N = t;
    H = 1;
    return true;
}

// per-target constants of the row passes (host-built, SlotInfo[A]): one 32-B
// uniform load per target instead of a chain of dependent graph lookups
struct alignas(16) SlotInfo {
    int32_t t;      // attached vertex (original id)
    int32_t c;      // relaxation vertex the row reads: t itself or its pendant anchor
    int32_t kt;     // full in-CSR entry of t's pendant edge, -1 if t is a relaxation vertex
    int32_t fast;   // 1: t's vertex factor is absent or 1.0 (no path-order re-fold for it)
    double pw;      // latency of the pendant edge (relaxation weight), 0 otherwise
    double pa;      // 1 - p of the pendant edge (get_eid edge), 1 otherwise
};

// Path-order sum 0.0 + a_1 + a_2 + ... of the auxiliary edge attribute along the
// row's path to core vertex c (then the pendant target edge kt, if any), as the
// offline completion tool sums a path's jitters (compute-topology-paths.py:27-33).
// The path is walked back from c through the parent edges; up to 64 core edges
// are kept and folded forward, longer paths re-walk per edge (O(h^2)).
template <int L>
__device__ double aux_fold(const DevGraph& G, const State& st, int32_t g, int32_t n, int32_t j, int32_t s,
                           int32_t c, int32_t kt) {
    constexpr int KMAX = 64;
    int32_t ks[KMAX];
    int32_t nk = 0;
    bool pend_src = false, overflow = false;
    for (int32_t x = c;;) {
        const int32_t k = st.P[sidx<L>(g, n, x, j)];
        if (k == -1) break;             // x is the (core) source
        if (k == -2) {                  // x is the anchor of a pruned source: s -> x
            pend_src = true;
            break;
        }
        if (nk < KMAX) ks[nk] = k;
        else overflow = true;
        ++nk;
        x = G.icol[k];
    }
    double a = 0.0;
    if (pend_src) a += G.fiaux[G.fiptr[s]];
    if (!overflow) {
        for (int32_t q = nk - 1; q >= 0; --q) a += G.iaux[ks[q]];
    } else {
        for (int32_t q = nk - 1; q >= 0; --q) {   // edge q (0 = the last one, into c)
            int32_t x = c;
            for (int32_t r = 0; r < q; ++r) x = G.icol[st.P[sidx<L>(g, n, x, j)]];
            a += G.iaux[st.P[sidx<L>(g, n, x, j)]];
        }
    }
    if (kt >= 0) a += G.fiaux[kt];
    return a;
}

// spe_table_opts.exact_delivery (DESIGN §4.1): the row kernels' DELIVERY = true
// instantiations test every routable entry of an offset row (a source without a
// relaxation lane of its own: a pruned pendant behind its anchor, a derived source
// behind a leg) with delivery_near_boundary and append the flagged ones to their 64-source
// block's worklist, which k_refold_delivery re-folds in path order.
struct Deliv {
    uint32_t* cnt;    // [block of the batch] flagged entries (keeps counting past the cap)
    int4* work;       // [block of the batch][cap] {source slot of the batch, target slot, root state
                      // lane, winning leg (index into the batch's legs) or -1: the pendant edge rwa[source]}
    int32_t cap;      // records per block: ceil(delivery_refold_max * 64 * A)
};
// spe_table_opts.delivery_refold_max = 0: half the flagged share at which re-folding a block
// entry by entry costs what rebuilding it one lane per source does (MEASUREMENTS.md)
#ifndef SPE_DELIVERY_REFOLD_DEFAULT
#define SPE_DELIVERY_REFOLD_DEFAULT 0.15
#endif
constexpr double DELIVERY_REFOLD_DEFAULT = SPE_DELIVERY_REFOLD_DEFAULT;

// One flagged entry per lane, every lane of the wave in block b (wave-uniform call):
// one atomic per wave takes the wave's positions, lanes below the cap store a record.
__device__ __forceinline__ void deliv_push(const Deliv& dv, int32_t b, bool flag, int32_t src, int32_t jt,
                                           int32_t root_lane, int32_t leg) {
    const uint64_t m = __ballot(flag);
    if (!m) return;
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int32_t leader = __builtin_ctzll(m);
    int32_t base = 0;
    if (lane == leader) base = (int32_t)atomicAdd(dv.cnt + b, (uint32_t)__builtin_popcountll(m));
    base = __shfl(base, leader);
    if (flag) {
        const uint32_t pos = (uint32_t)base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (pos < (uint32_t)dv.cap) dv.work[(size_t)b * (size_t)dv.cap + pos] = make_int4(src, jt, root_lane, leg);
    }
}

// State -> table rows.  One wave per (64-source block of the batch, target
// slot): lane l = source b*64 + l, i.e. lane group b*(64/L) + l/L, lane l%L.
#ifndef ROWS_ITEMS
#define ROWS_ITEMS 2
#endif
// SHARE (shared anchor trees): the state lanes are the batch's roots; rli[b * 64 + l]
// = {state lane of source b * 64 + l's root, its first hop (the anchor) or -1 for a
// core source} and rwa[.] = {pendant edge latency w, f_s * (1 - p)}: a pruned pendant
// source's row is its anchor's with the edge folded in front (latency w + d,
// reliability (f_s a) r, one more hop, first hop the anchor).
// (Here only for contracted shared tables; plain ones take k_rows_shared_lds.)
template <int L, bool AUX, bool SHARE = false, bool DELIVERY = false>
__global__ __launch_bounds__(BLOCK) void k_rows_sssp(int32_t n, int32_t blocks, int32_t sb0,
                                                     const int32_t* __restrict__ srcv,
                                                     const SlotInfo* __restrict__ slots, DevGraph G,
                                                     RowMode md, State st, Table tb,
                                                     const int2* __restrict__ rli = nullptr,
                                                     const double2* __restrict__ rwa = nullptr,
                                                     Deliv dv = Deliv{nullptr, nullptr, 0}) {
    static_assert(!DELIVERY || SHARE, "only shared rows carry an offset");
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int64_t items_all = (int64_t)blocks * tb.A;
    // XCD-contiguous slices (grid a multiple of 8; workgroups are dealt round-robin
    // over the 8 XCDs): one XCD's waves take consecutive items, so targets that
    // share a pendant anchor (adjacent slots) read that anchor's state row from
    // the same L2 instead of one XCD each.
    const bool xs = (gridDim.x & 7) == 0;
    const int32_t xcd = xs ? (int32_t)(blockIdx.x & 7) : 0;
    const int64_t nwaves = xs ? (((int64_t)(gridDim.x >> 3) * BLOCK) >> 6) : (((int64_t)gridDim.x * BLOCK) >> 6);
    const int64_t lo = xs ? items_all * xcd / 8 : 0;
    const int64_t items = xs ? items_all * (xcd + 1) / 8 : items_all;
    const int64_t wave0 = xs ? ((((int64_t)(blockIdx.x >> 3) * BLOCK + threadIdx.x) >> 6))
                             : ((((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6));
    // Two items per trip: every load both need (slot constants, source, the
    // target row's distance and route) is issued before either one's stores,
    // so a trip waits for two memory round trips, not four.
    struct In {
        int32_t b, jt, s;
        SlotInfo si;
        double dc;
        Route rc;
        int2 ri;       // SHARE: (root's state lane, first hop of a pendant source or -1)
    };
    constexpr int NI = ROWS_ITEMS;
    // SHARE: items run over tiles of BT consecutive source blocks, the blocks fastest:
    // the ~10 blocks whose sources share one lane group of roots then read a target's
    // root row from L2 one after the other instead of once per block sweep (each
    // item still writes one whole 1-KB record segment)
    constexpr int BT = SHARE ? 8 : 1;
    auto load1 = [&](int64_t i0, In (&dst)[NI]) {
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int64_t it = i0 + q * nwaves;
            In& x = dst[q];
            x.b = -1;
            if (it < items) {
                if constexpr (BT > 1) {
                    const int64_t tile = it / ((int64_t)BT * tb.A);
                    const int32_t b0 = (int32_t)tile * BT;
                    const int32_t bt = min(BT, blocks - b0);
                    const int64_t r = it - tile * BT * (int64_t)tb.A;
                    x.jt = (int32_t)(r / bt);
                    x.b = b0 + (int32_t)(r - (int64_t)x.jt * bt);
                } else {
                    x.b = (int32_t)(it / tb.A);
                    x.jt = (int32_t)(it - (int64_t)x.b * tb.A);
                }
                x.si = slots[x.jt];
                x.s = srcv[x.b * WAVE + lane];
                if constexpr (SHARE) x.ri = rli[x.b * WAVE + lane];
            }
        }
    };
    for (int64_t it0 = lo + wave0; it0 < items; it0 += NI * nwaves) {
        In in[NI];
        load1(it0, in);
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            In& x = in[q];
            x.dc = INF;
            if (x.b >= 0 && x.s >= 0 && x.si.t != x.s) {
                const int32_t sl = SHARE ? x.ri.x : x.b * WAVE + lane;   // state lane
                const int32_t g = sl / L, j = sl % L;
                if (x.si.c >= 0) {
                    const size_t rt = sidx<L>(g, n, x.si.c, j);
                    x.dc = st.D[rt];
                    x.rc = st.RT[rt];
                } else {   // a contracted target: the best of its three neighbours (d, then d[u], then u)
                    const int32_t r = -2 - x.si.c;
                    const int32_t u0 = G.rnb[3 * r], u1 = G.rnb[3 * r + 1], u2 = G.rnb[3 * r + 2];
                    const double d0 = st.D[sidx<L>(g, n, u0, j)], d1 = st.D[sidx<L>(g, n, u1, j)],
                                 d2 = st.D[sidx<L>(g, n, u2, j)];
                    const double a0 = d0 + G.rw[3 * r], a1 = d1 + G.rw[3 * r + 1], a2 = d2 + G.rw[3 * r + 2];
                    int32_t q = d0 < INF ? 0 : -1;
                    double bd = d0 < INF ? a0 : INF, bu = d0;
                    const bool t1 = (d1 < INF) & ((a1 < bd) | ((a1 == bd) & (d1 < bu)));   // (branch-free: lex_less3)
                    q = t1 ? 1 : q;
                    bd = t1 ? a1 : bd;
                    bu = t1 ? d1 : bu;
                    const bool t2 = (d2 < INF) & ((a2 < bd) | ((a2 == bd) & (d2 < bu)));
                    q = t2 ? 2 : q;
                    bd = t2 ? a2 : bd;
                    bu = t2 ? d2 : bu;
                    if (q >= 0) {
                        const Route rc = st.RT[sidx<L>(g, n, G.rnb[3 * r + q], j)];
                        x.dc = bd;
                        x.rc.r = rc.r * G.ra[3 * r + q];
                        x.rc.h = rc.h + 1;
                        x.rc.f = (rc.h == 0) ? x.si.t : rc.f;   // the neighbour is the source itself
                    }
                }
                if constexpr (SHARE) {
                    if (x.ri.y >= 0 && x.dc < INF) {   // a pruned pendant source: s -> anchor, then the root's path
                        const double2 wa = rwa[x.b * WAVE + lane];
                        x.dc = wa.x + x.dc;
                        x.rc.r = wa.y * x.rc.r;
                        x.rc.h = x.rc.h + 1;
                        x.rc.f = x.ri.y;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const In& x = in[q];
            if (x.b < 0) continue;
            const int32_t b = x.b, jt = x.jt, s = x.s;
            const SlotInfo& si = x.si;
            const int32_t t = si.t;
            const int32_t g = (b * WAVE + lane) / L, j = (b * WAVE + lane) % L;   // (!SHARE: the re-fold walks)
            double Lt = -1.0, R = -1.0, AX = -1.0;
            int32_t N = -1, H = 0, PV = -1;
            if (s >= 0) {
                if (t == s) {
                    self_entry(G, md, s, Lt, R, N, H);
                    PV = (H == 2) ? N : (H > 0 ? s : -1);
                    AX = 0.0;
                } else {
                    // a pruned pendant target is one edge past its anchor: Dijkstra's
                    // d[t] = d[c] + w, parent c (its only candidate)
                    const int32_t c = si.c;
                    const int32_t kt = si.kt;
                    const size_t rt = sidx<L>(g, n, c, j);
                    const double dc = x.dc;
                    if (dc < INF) {
                        const Route rc = x.rc;
                        double d = dc;
                        Route rr = rc;
                        if (kt >= 0) {
                            d = dc + si.pw;
                            rr.r = rc.r * si.pa;
                            rr.h = rc.h + 1;
                            rr.f = (rc.h == 0) ? t : rc.f;   // c is the source itself
                        }
                        const bool fast = si.fast && !md.multi_rep;
                        if (fast) {
                            Lt = d;
                            R = rr.r;
                        } else {
                            // path-order re-fold, shd-topology.c:1413-1493 (rare: vertex loss on
                            // the target, or multigraph get_eid latencies).  Edge i of the path
                            // (1 = leaves the source) is found by walking back from t.
                            const double fs = G.vfac[s];
                            const double ft = G.vfac[t];
                            double l = 0.0, r = 1.0;
                            if (has_attr(fs)) r *= fs;
                            if (has_attr(ft)) r *= ft;
                            const int32_t h = rr.h;
                            for (int32_t i = 1; i <= h; ++i) {
                                int32_t back = h - i;   // edges to step over from the end
                                double ew, ea;
                                if (kt >= 0 && back == 0) {
                                    ew = G.fiwrep[kt];
                                    ea = G.fia[kt];
                                } else {
                                    int32_t x = c;
                                    if (kt >= 0) back -= 1;
                                    for (int32_t q = 0; q < back; ++q) x = G.icol[st.P[sidx<L>(g, n, x, j)]];
                                    const int32_t k = st.P[sidx<L>(g, n, x, j)];
                                    if (k >= 0) {
                                        ew = G.iwrep[k];
                                        ea = G.ia[k];
                                    } else {   // -2: the pendant source's edge into its anchor
                                        ew = G.fiwrep[G.fiptr[s]];
                                        ea = G.fia[G.fiptr[s]];
                                    }
                                }
                                l += ew;
                                r *= ea;
                            }
                            Lt = l;
                            R = r;
                        }
                        if (Lt == 0) Lt = 1;   // shd-topology.c:1833-1837
                        if constexpr (AUX) AX = aux_fold<L>(G, st, g, n, j, s, c, kt);
                        N = rr.f;
                        H = rr.h;
                        if (tb.prev) {
                            if (kt >= 0) {
                                PV = G.corev[c];
                            } else {
                                const int32_t pk = st.P[rt];
                                PV = pk >= 0 ? G.corev[G.icol[pk]] : s;   // -2: parent is the pendant source
                            }
                        }
                    }
                }
            }
            if constexpr (DELIVERY) {   // a pendant source's routable entry: offset by its edge
                const bool off = s >= 0 && t != s && x.ri.y >= 0 && x.dc < INF;
                deliv_push(dv, b, off && delivery_near_boundary(Lt, H), b * WAVE + lane, jt, x.ri.x, -1);
            }
            const size_t o = tidx(sb0 + b, tb.A, jt, lane);
            // the table is written once and not read during the build: stream it
            dvec2 e;
            e.x = Lt;
            e.y = R;
            __builtin_nontemporal_store(e, reinterpret_cast<dvec2*>(tb.lr + o));
            __builtin_nontemporal_store(N, tb.next + o);
            __builtin_nontemporal_store((uint16_t)(H > 65535 ? 65535 : H), tb.hops + o);
            if (tb.prev) tb.prev[o] = PV;
            if constexpr (AUX) tb.aux[o] = AX;
        }
    }
}


// Shared anchor trees, rows through LDS (plain relaxation graph, fast targets): a
// workgroup takes a tile of RT_B (16) consecutive source blocks x RT_T (4) consecutive
// targets.  The tile's sources read the root lanes [r0, r1] (rng[tile], host-built;
// roots are numbered in first-appearance order, so a tile's ~100 roots are
// consecutive lanes), so the workgroup first stages those lanes' distance and route
// for its RT_T targets in LDS -- every load of the tile in flight at once, one
// memory round trip -- and then writes the tile's 64-lane records from LDS (each
// wave one source block's targets in order: contiguous 1-KB record segments).
// A tile whose lane span exceeds RT_R takes the per-lane gathers of k_rows_sssp.
#ifndef SPE_RT_B
#define SPE_RT_B 16
#endif
#ifndef SPE_RT_T
#define SPE_RT_T 4
#endif
constexpr int RT_B = SPE_RT_B, RT_T = SPE_RT_T, RT_R = 24 * SPE_RT_B;

template <int L, bool DELIVERY = false>
__global__ __launch_bounds__(BLOCK) void k_rows_shared_lds(int32_t n, int32_t blocks, int32_t sb0,
                                                           const int32_t* __restrict__ srcv,
                                                           const SlotInfo* __restrict__ slots, DevGraph G,
                                                           RowMode md, State st, Table tb,
                                                           const int2* __restrict__ rli,
                                                           const double2* __restrict__ rwa,
                                                           const int2* __restrict__ rng,
                                                           Deliv dv = Deliv{nullptr, nullptr, 0}) {
    __shared__ double sD[RT_T][RT_R];
    __shared__ Route sR[RT_T][RT_R];
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int32_t wib = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
    const int32_t ntiles = (blocks + RT_B - 1) / RT_B;
    const int32_t ntc = (tb.A + RT_T - 1) / RT_T;
    const int64_t work = (int64_t)ntiles * ntc;
    for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {   // workgroup-uniform
        const int32_t tile = (int32_t)(w / ntc);
        const int32_t jt0 = (int32_t)(w - (int64_t)tile * ntc) * RT_T;
        const int32_t b0 = tile * RT_B, nb = min(RT_B, blocks - b0);
        const int32_t nt = min(RT_T, tb.A - jt0);
        const int2 rr = rng[tile];
        const int32_t nr = rr.y - rr.x + 1;
        const bool staged = nr > 0 && nr <= RT_R;
        if (staged) {
            for (int32_t i = threadIdx.x; i < nt * nr; i += BLOCK) {
                const int32_t tl = i / nr, q = i - tl * nr;
                const int32_t c = slots[jt0 + tl].c;
                const int32_t R = rr.x + q;
                double d = INF;
                Route rt{1.0, 0, -1};
                if (c >= 0) {
                    const size_t x = sidx<L>(R / L, n, c, R % L);
                    d = st.D[x];
                    rt = st.RT[x];
                }
                sD[tl][q] = d;
                sR[tl][q] = rt;
            }
        }
        __syncthreads();
        for (int32_t bl = wib; bl < nb; bl += BLOCK / WAVE) {
            const int32_t b = b0 + bl;
            const int32_t s = srcv[b * WAVE + lane];
            const int2 ri = rli[b * WAVE + lane];
            const double2 wa = rwa[b * WAVE + lane];
            for (int32_t tl = 0; tl < nt; ++tl) {
                const int32_t jt = jt0 + tl;
                const SlotInfo si = slots[jt];
                double Lt = -1.0, R = -1.0;
                int32_t N = -1, H = 0;
                bool off = false;   // (DELIVERY) a routable entry of a pendant source
                (void)off;
                if (s >= 0) {
                    if (si.t == s) {
                        self_entry(G, md, s, Lt, R, N, H);
                    } else {
                        double dc = INF;
                        Route rc{1.0, 0, -1};
                        if (staged) {
                            dc = sD[tl][ri.x - rr.x];
                            rc = sR[tl][ri.x - rr.x];
                        } else if (si.c >= 0) {
                            const size_t x = sidx<L>(ri.x / L, n, si.c, ri.x % L);
                            dc = st.D[x];
                            rc = st.RT[x];
                        }
                        if (dc < INF) {
                            if (ri.y >= 0) {   // a pruned pendant source: s -> anchor, then the root's path
                                dc = wa.x + dc;
                                rc.r = wa.y * rc.r;
                                rc.h = rc.h + 1;
                                rc.f = ri.y;
                                if constexpr (DELIVERY) off = true;
                            }
                            double d = dc;
                            Route rt2 = rc;
                            if (si.kt >= 0) {   // a pruned pendant target: one edge past its anchor
                                d = dc + si.pw;
                                rt2.r = rc.r * si.pa;
                                rt2.h = rc.h + 1;
                                rt2.f = (rc.h == 0) ? si.t : rc.f;
                            }
                            Lt = d == 0 ? 1.0 : d;   // shd-topology.c:1833-1837
                            R = rt2.r;
                            N = rt2.f;
                            H = rt2.h;
                        }
                    }
                }
                if constexpr (DELIVERY)
                    deliv_push(dv, b, off && delivery_near_boundary(Lt, H), b * WAVE + lane, jt, ri.x, -1);
                const size_t o = tidx(sb0 + b, tb.A, jt, lane);
                dvec2 e;
                e.x = Lt;
                e.y = R;
                __builtin_nontemporal_store(e, reinterpret_cast<dvec2*>(tb.lr + o));
                __builtin_nontemporal_store(N, tb.next + o);
                __builtin_nontemporal_store((uint16_t)(H > 65535 ? 65535 : H), tb.hops + o);
            }
        }
        __syncthreads();   // the next tile's staging overwrites sD / sR
    }
}

// Contracted shared tables: derived rows (DESIGN §4.1).  The relaxation lanes are
// the batch's roots (kept core sources, pendant anchors); a derived source x takes
// no lane: every path from x starts with one of its LEGS -- a one- or two-edge
// prefix ending at a kept vertex u whose lane is read, or a direct edge to one
// target -- so
//   d_x(t) = min over legs fl(w_leg + d_u(t)),  next hop = the leg's first hop,
//   hops = the leg's edges + h_u(t), reliability a_leg r_u(t)
// (shd-topology.c:1741 runs one Dijkstra per source instead).  Legs (host-built,
// spe_graph_prep.cpp contract_degree3): a removed degree-3 vertex's three edges; a
// derived kept vertex's contracted entries read from it (x -> u, x -> y -> b through
// a removed y) plus the direct edge to y; a removed vertex next to a derived kept x
// reaches x's plain neighbours through x (y -> x -> k) and x itself directly.  Core
// sources have one leg (their own lane, no prefix), pendant sources one (the
// anchor's lane behind the pendant edge).  x's route is the winning leg's route
// exactly when that leg wins by more than the rounding the sums carry and the
// lane's own decisions hold for the offset (k_share_check); a source where the first
// test fails is flagged in `sunsafe` and its block is rebuilt one lane per source.
// A removed TARGET y reads its three neighbours in the root's row (best by (d, d[u],
// u), k_expand_removed); for a source with an offset that choice is margin-checked
// too.  Items are (chunk of TC tiles of TT targets, source block), target chunks
// slowest and XCD-contiguous: an XCD's resident waves work on the same few targets,
// so the state columns the derived sources gather stay in that XCD's L2.
struct alignas(16) DLeg {
    double w;         // prefix latency, path order from the source (0: a core source's own lane)
    int32_t ref;      // root lane the leg reads (>= 0); < 0: a direct edge reaching the one target
                      // whose relaxation code is leg_direct_tc(ref)
    int32_t pad0;
    double a;         // prefix reliability factor, path order (a pendant source's f_s folded in)
    int32_t hopinc;   // first hop (original id) | prefix edges << 29; -1: no prefix (core source)
    int32_t pad1;
};

// direct legs: the target code c (SlotInfo.c: kept id >= 0, or -2 - removed index) <-> ref < 0
__host__ __device__ __forceinline__ int32_t leg_direct_ref(int32_t c) {
    return -1 - (c >= 0 ? 2 * c : 2 * (-2 - c) + 1);
}
__device__ __forceinline__ int32_t leg_direct_tc(int32_t ref) {
    const int32_t code = -1 - ref;
    return (code & 1) ? -2 - (code >> 1) : (code >> 1);
}

__device__ __forceinline__ bool near_tie(double best, double alt, double wmin, double omax, double hmax) {
    const double h = wmin > 0.0 ? fmin(hmax, alt / wmin + 3.0) : hmax;
    return alt - best <= 4.5 * h * 0x1p-53 * (omax + alt);
}

// A root lane's value at a target: the relaxation vertex c's distance, or for a
// removed target (c = -2 - r) the expanded entry k_expand_removed wrote (the best
// of its three neighbours, its sign the margin flag); `tight` when an offset could
// change that choice (runner-up within the margin of k_share_check) -- only asked
// for sources with an offset.
struct RootVal {
    double d;
    bool tight;
};

template <int L>
__device__ __forceinline__ RootVal root_val(const double* __restrict__ SD, const double* __restrict__ DX, int32_t n,
                                            int32_t nr, int32_t sl, int32_t c, bool check) {
    RootVal o;
    const int32_t g = sl / L, j = sl - (sl / L) * L;
    if (c >= 0) {
        o.d = SD[sidx<L>(g, n, c, j)];
        o.tight = false;
    } else {
        const double x = DX[sidx<L>(g, nr, -2 - c, j)];
        o.d = __builtin_fabs(x);
        o.tight = check && __builtin_signbit(x);
    }
    return o;
}

// the route record a row continues: the relaxation state's, or a removed target's
// expanded one (the edge past the neighbour already folded in)
template <int L>
__device__ __forceinline__ const Route* root_route(const Route* __restrict__ SRT, const Route* __restrict__ RTX,
                                                   int32_t n, int32_t nr, int32_t sl, int32_t c) {
    const int32_t g = sl / L, j = sl - (sl / L) * L;
    return c >= 0 ? SRT + sidx<L>(g, n, c, j) : RTX + sidx<L>(g, nr, -2 - c, j);
}

// Contracted shared tables: every (root lane, removed vertex) entry once, before the
// rows -- the best of the removed vertex's three neighbours by (d, d[u], u) as
// k_rows_sssp chooses it, with the route one edge past that neighbour, and (sums
// not exact) the sign bit set when a runner-up is within the margin of an offset
// source (near_tie).  The rows kernel then reads one entry where every source that
// reads the lane (its own, and each derived source next to it: a hub's lane is read
// by thousands) re-did three gathers and the choice.  One wave per (lane group,
// removed vertex): three coalesced neighbour rows in, one row of DX and of RTX out.
template <int L>
__global__ __launch_bounds__(BLOCK) void k_expand_removed(int32_t groups, int32_t n, int32_t nr, DevGraph G, State st,
                                                          double* __restrict__ DX, Route* __restrict__ RTX,
                                                          const int32_t* __restrict__ rorig, int32_t check,
                                                          double wmin, double omax, double hmax) {
    constexpr int M = L / WAVE;
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int64_t items = (int64_t)groups * nr;
    const int64_t nw = ((int64_t)gridDim.x * BLOCK) >> 6;
    for (int64_t it = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6; it < items; it += nw) {   // wave-uniform
        const int32_t g = (int32_t)(it / nr), r = (int32_t)(it - (it / nr) * nr);
        const int32_t u0 = G.rnb[3 * r], u1 = G.rnb[3 * r + 1], u2 = G.rnb[3 * r + 2];
        const double w0 = G.rw[3 * r], w1 = G.rw[3 * r + 1], w2 = G.rw[3 * r + 2];
        double d0[M], d1[M], d2[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int32_t j = lane + m * WAVE;
            d0[m] = st.D[sidx<L>(g, n, u0, j)];
            d1[m] = st.D[sidx<L>(g, n, u1, j)];
            d2[m] = st.D[sidx<L>(g, n, u2, j)];
        }
        int32_t qq[M];
        double bb[M];
        bool tt[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double a0 = d0[m] + w0, a1 = d1[m] + w1, a2 = d2[m] + w2;
            int32_t q = d0[m] < INF ? 0 : -1;
            double bd = d0[m] < INF ? a0 : INF, bu = d0[m];
            const bool t1 = (d1[m] < INF) & ((a1 < bd) | ((a1 == bd) & (d1[m] < bu)));   // (branch-free: lex_less3)
            q = t1 ? 1 : q;
            bd = t1 ? a1 : bd;
            bu = t1 ? d1[m] : bu;
            const bool t2 = (d2[m] < INF) & ((a2 < bd) | ((a2 == bd) & (d2[m] < bu)));
            q = t2 ? 2 : q;
            bd = t2 ? a2 : bd;
            bool t = false;
            if (check && q >= 0) {
                if (q != 0 && d0[m] < INF) t |= near_tie(bd, a0, wmin, omax, hmax);
                if (q != 1 && d1[m] < INF) t |= near_tie(bd, a1, wmin, omax, hmax);
                if (q != 2 && d2[m] < INF) t |= near_tie(bd, a2, wmin, omax, hmax);
            }
            qq[m] = q;
            bb[m] = bd;
            tt[m] = t;
        }
        Route rc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            rc[m] = Route{1.0, 0, -1};
            if (qq[m] >= 0) rc[m] = st.RT[sidx<L>(g, n, qq[m] == 0 ? u0 : (qq[m] == 1 ? u1 : u2), lane + m * WAVE)];
        }
        const int32_t yo = rorig[r];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const size_t o = sidx<L>(g, nr, r, lane + m * WAVE);
            Route x = rc[m];
            if (qq[m] >= 0) {   // one edge past the neighbour taken
                x.r = rc[m].r * G.ra[3 * r + qq[m]];
                x.h = rc[m].h + 1;
                x.f = (rc[m].h == 0) ? yo : rc[m].f;   // the neighbour is the lane's root itself
            }
            DX[o] = qq[m] < 0 ? INF : (tt[m] ? -bb[m] : bb[m]);
            RTX[o] = x;
        }
    }
}

#ifndef SPE_DERIVED_TT
#define SPE_DERIVED_TT 3
#endif
// Each item's TT targets go through the load chain together -- slot constants
// (scalar), then every leg's root value, then the winners' route records -- so a
// wave waits for a few memory round trips per tile, not per target (the stores
// could alias the state as far as the compiler knows, so target-at-a-time code
// serialises every target's chain behind the last one's stores).  The first KR legs
// of each source stay in registers for the whole item; more legs (derived kept
// vertices and their removed neighbours: up to ~10) are read per tile.
#ifndef SPE_DERIVED_OCC
#define SPE_DERIVED_OCC 1
#endif
// An item is (chunk of TC tiles of TT targets, source block): the block's source
// constants are loaded once per chunk (A/B, C3: TC 1 / 4 / 16 / 64 -> 56 / 52 / 60 /
// 63 ms of rows per table: larger chunks lose the XCD's column locality).
#ifndef SPE_DERIVED_TC
#define SPE_DERIVED_TC 4
#endif
// f(o) = o - margin(o): a competing first leg o is a near tie of the best b iff
// f(o) <= b (near_tie; exact sums: only an exact tie)
__device__ __forceinline__ double tie_floor(double o, double wmin, double omax, double hmax, int32_t exact) {
    if (exact) return o;
    const double h = wmin > 0.0 ? fmin(hmax, o / wmin + 3.0) : hmax;
    return o - 4.5 * h * 0x1p-53 * (omax + o);
}

// GEN = false: no target of the table is a pruned pendant and the self entries are
// written afterwards by k_rows_self -- the two rare paths cost 27 VGPRs when
// inlined (145 -> 116: 3 -> 4 waves / SIMD for this latency-bound kernel).
template <int L, int TT, int TC = SPE_DERIVED_TC, bool GEN = true>
__global__ __launch_bounds__(BLOCK, SPE_DERIVED_OCC) void k_rows_derived(int32_t n, int32_t blocks, int32_t sb0,
                                                        const int32_t* __restrict__ srcv,
                                                        const SlotInfo* __restrict__ slots, DevGraph G,
                                                        RowMode md, const double* __restrict__ SD,
                                                        const Route* __restrict__ SRT, Table tb,
                                                        const int2* __restrict__ lrng,
                                                        const DLeg* __restrict__ legs,
                                                        const double* __restrict__ DX,
                                                        const Route* __restrict__ RTX, int32_t nr, double wmin,
                                                        double omax, double hmax, int32_t exact,
                                                        uint8_t* __restrict__ sunsafe) {
#ifndef SPE_DERIVED_KR
#define SPE_DERIVED_KR 3   // legs per source held in registers for the whole item (more: re-read per tile; A/B 3 / 4 -> 71.0 / 72.2 ms)
#endif
    constexpr int KR = SPE_DERIVED_KR;
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int32_t ntt = (tb.A + TT - 1) / TT;
    const int32_t nch = (ntt + TC - 1) / TC;
    const int64_t items_all = (int64_t)nch * blocks;
    const bool xs = (gridDim.x & 7) == 0;
    const int32_t xcd = xs ? (int32_t)(blockIdx.x & 7) : 0;
    const int64_t nwaves = xs ? (((int64_t)(gridDim.x >> 3) * BLOCK) >> 6) : (((int64_t)gridDim.x * BLOCK) >> 6);
    const int64_t lo = xs ? items_all * xcd / 8 : 0;
    const int64_t items = xs ? items_all * (xcd + 1) / 8 : items_all;
    const int64_t wave0 = xs ? ((((int64_t)(blockIdx.x >> 3) * BLOCK + threadIdx.x) >> 6))
                             : ((((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6));
    for (int64_t it = lo + wave0; it < items; it += nwaves) {   // wave-uniform
        const int32_t ch = (int32_t)(it / blocks);
        const int32_t b = (int32_t)(it - (int64_t)ch * blocks);
        const int32_t s = srcv[b * WAVE + lane];
        const int2 lr = lrng[b * WAVE + lane];
        const int32_t nl = s >= 0 ? (lr.y & 0xFFFF) : 0;     // legs (0: padding)
        const bool chk = (lr.y >> 16) != 0 && !exact;       // an offset source: margins checked
        int32_t nlmax = nl;
        for (int o = 32; o > 0; o >>= 1) nlmax = max(nlmax, __shfl_xor(nlmax, o));
        nlmax = __builtin_amdgcn_readfirstlane(nlmax);
        DLeg lg[KR];
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < nl) {
                lg[k] = legs[lr.x + k];
            } else {
                lg[k].w = INF;
                lg[k].a = 1.0;
                lg[k].ref = INT32_MAX;   // no leg
                lg[k].hopinc = -1;
            }
        }
        bool bad = false;
        for (int32_t tt = ch * TC; tt < min(ntt, (ch + 1) * TC); ++tt) {   // wave-uniform
            SlotInfo si[TT];
            int32_t sc[TT];
            bool live[TT];
#pragma unroll
            for (int tl = 0; tl < TT; ++tl) {
                const int32_t jt = tt * TT + tl;
                si[tl] = slots[jt < tb.A ? jt : tb.A - 1];
                sc[tl] = si[tl].c;
                live[tl] = jt < tb.A && s >= 0 && si[tl].t != s;
            }
            double bo[TT], m2[TT];
            int32_t bi[TT];
            bool tg[TT];
#pragma unroll
            for (int tl = 0; tl < TT; ++tl) {
                bo[tl] = INF;
                m2[tl] = INF;
                bi[tl] = 0;
                tg[tl] = false;
            }
            for (int32_t k0 = 0; k0 < nlmax; k0 += KR) {   // wave-uniform
                int32_t rr[KR];
                double ww[KR];
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k0 == 0) {
                        rr[k] = lg[k].ref;
                        ww[k] = lg[k].w;
                    } else if (k0 + k < nl) {
                        const DLeg d = legs[lr.x + k0 + k];
                        rr[k] = d.ref;
                        ww[k] = d.w;
                    } else {
                        rr[k] = INT32_MAX;
                        ww[k] = INF;
                    }
                }
                RootVal v[TT][KR];
#pragma unroll
                for (int tl = 0; tl < TT; ++tl)
#pragma unroll
                    for (int k = 0; k < KR; ++k) {
                        v[tl][k].d = INF;
                        v[tl][k].tight = false;
                        if (!live[tl] || rr[k] == INT32_MAX) continue;
                        if (rr[k] >= 0) v[tl][k] = root_val<L>(SD, DX, n, nr, rr[k], sc[tl], chk);
                        else if (leg_direct_tc(rr[k]) == sc[tl]) v[tl][k].d = 0.0;
                    }
                // running best first leg (strict: the first of equal sums wins; a tie
                // flags the source anyway) and the lowest tie floor of the others
#pragma unroll
                for (int tl = 0; tl < TT; ++tl)
#pragma unroll
                    for (int k = 0; k < KR; ++k) {
                        const double o = ww[k] + v[tl][k].d;
                        if (!(o < INF)) continue;
                        const bool better = o < bo[tl];
                        const double loser = better ? bo[tl] : o;
                        if (loser < INF) m2[tl] = fmin(m2[tl], tie_floor(loser, wmin, omax, hmax, exact));
                        bo[tl] = better ? o : bo[tl];
                        bi[tl] = better ? k0 + k : bi[tl];
                        tg[tl] = better ? v[tl][k].tight : tg[tl];
                    }
            }
            // the winners' legs (registers for the first KR) and route records
            Route rc[TT];
            double ap[TT];
            int32_t hi[TT];
#pragma unroll
            for (int tl = 0; tl < TT; ++tl) {
                rc[tl] = Route{1.0, 0, -1};
                ap[tl] = 1.0;
                hi[tl] = -1;
                if (!(bo[tl] < INF)) continue;
                if (nl > 1) bad |= m2[tl] <= bo[tl];   // u* must beat the other first legs by more than rounding
                bad |= tg[tl];
                int32_t ref = 0;
                if (bi[tl] < KR) {
#pragma unroll
                    for (int k = 0; k < KR; ++k) {
                        ref = k == bi[tl] ? lg[k].ref : ref;
                        ap[tl] = k == bi[tl] ? lg[k].a : ap[tl];
                        hi[tl] = k == bi[tl] ? lg[k].hopinc : hi[tl];
                    }
                } else {
                    const DLeg d = legs[lr.x + bi[tl]];
                    ref = d.ref;
                    ap[tl] = d.a;
                    hi[tl] = d.hopinc;
                }
                if (ref >= 0) rc[tl] = *root_route<L>(SRT, RTX, n, nr, ref, sc[tl]);
            }
#pragma unroll
            for (int tl = 0; tl < TT; ++tl) {
                const int32_t jt = tt * TT + tl;
                if (jt >= tb.A) break;
                const SlotInfo& sv = si[tl];
                double Lt = -1.0, R = -1.0;
                int32_t N = -1, H = 0;
                if (s >= 0) {
                    if (GEN && sv.t == s) {
                        self_entry(G, md, s, Lt, R, N, H);
                    } else if (bo[tl] < INF) {
                        double d = bo[tl];
                        Route rt = rc[tl];
                        if (hi[tl] >= 0) {   // a prefix in front: its edges, its first hop
                            rt.r = ap[tl] * rt.r;
                            rt.h = rt.h + (hi[tl] >> 29);
                            rt.f = hi[tl] & 0x1FFFFFFF;
                        }
                        if (GEN && sv.kt >= 0) {   // a pruned pendant target: one edge past its anchor
                            d = d + sv.pw;
                            rt.r = rt.r * sv.pa;
                            rt.f = (rt.h == 0) ? sv.t : rt.f;
                            rt.h = rt.h + 1;
                        }
                        Lt = d == 0 ? 1.0 : d;   // shd-topology.c:1833-1837
                        R = rt.r;
                        N = rt.f;
                        H = rt.h;
                    }
                }
                const size_t o = tidx(sb0 + b, tb.A, jt, lane);
                dvec2 e;
                e.x = Lt;
                e.y = R;
                __builtin_nontemporal_store(e, reinterpret_cast<dvec2*>(tb.lr + o));
                __builtin_nontemporal_store(N, tb.next + o);
                __builtin_nontemporal_store((uint16_t)(H > 65535 ? 65535 : H), tb.hops + o);
            }
        }   // target tiles of the chunk
        if (bad) sunsafe[b * WAVE + lane] = 1;
    }
}


// ---- Lane-major derived rows (SPE_ROWS_LM).  k_rows_derived gathers one 8-B value per
// (source lane, leg) from 64 different state lines per instruction, so the texture
// addresser spends a cycle per lane (r04 counters: TA ~80 % busy, ~60 TA cycles per
// VMEM instruction).  Here the root lanes are first staged lane-major per target
// slot (k_stage_lanes: XD[lane][t], the distance or a removed target's expanded
// entry with its margin sign, XRT[lane][t] the route), and the rows kernel puts 32
// consecutive TARGETS on the lanes of a half-wave: a leg's values are one coalesced
// 256-B load, the winner's routes a few lines; the records of a 64-source block x
// 32 targets are transposed through LDS into the SB64 segments.
#ifndef SPE_ROWS_LM
#define SPE_ROWS_LM 1   // lane-major derived rows (k_stage_lanes + k_rows_lm); 0: k_rows_derived
#endif
#ifndef SPE_LM_T
#define SPE_LM_T 16     // targets per rows item (a divisor of 64: 64 / LM_T sources per wave step;
                        // A/B on C3: 16 / 32 -> 39.9 / 41.4 ms with the preload)
#endif
constexpr int LM_T = SPE_LM_T;
#ifndef SPE_LM_TS
#define SPE_LM_TS 16   // target slots per staging item (k_stage_lanes' LDS tile: 3.3 KB per slot)
#endif
constexpr int LM_TS = SPE_LM_TS;
__host__ __device__ constexpr int64_t lm_stride(int32_t A) { return ((int64_t)A + LM_T - 1) / LM_T * LM_T; }

#ifndef SPE_LM_FUSE
#define SPE_LM_FUSE 1   // k_stage_lanes expands removed targets itself (no k_expand_removed, no DX / RTX)
#endif
__global__ __launch_bounds__(BLOCK) void k_stage_lanes(int32_t groups, int32_t n, int32_t nr, int32_t A,
                                                       const SlotInfo* __restrict__ slots,
                                                       const double* __restrict__ SD, const Route* __restrict__ SRT,
                                                       const double* __restrict__ DX, const Route* __restrict__ RTX,
                                                       double* __restrict__ XD, Route* __restrict__ XRT, DevGraph G,
                                                       const int32_t* __restrict__ rorig, int32_t check, double wmin,
                                                       double omax, double hmax) {
    constexpr int L = 2 * WAVE, TS = LM_TS, TP = TS + 1;
    __shared__ double sD[L][TP];
    __shared__ Route sR[L][TP];
    const int32_t lane = threadIdx.x & (WAVE - 1), wib = threadIdx.x >> 6;
    const int64_t AP = lm_stride(A);
    const int32_t ntile = (A + TS - 1) / TS;
    const int64_t items = (int64_t)groups * ntile;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {   // workgroup-uniform
        const int32_t g = (int32_t)(it / ntile), t0 = (int32_t)(it - (it / ntile) * ntile) * TS;
        // a wave's QW targets go through the load chain together: every kept target's
        // distance and route and every removed target's three neighbour distances in
        // one round trip, then the removed targets' chosen routes
        constexpr int QW = TS / (BLOCK / WAVE);
        int32_t cq[QW];
        bool okq[QW];
#pragma unroll
        for (int q = 0; q < QW; ++q) {
            const int32_t t = t0 + wib + q * (BLOCK / WAVE);
            okq[q] = t < A;
            cq[q] = okq[q] ? slots[t].c : 0;
        }
        double dv[QW][2], e1[QW][2], e2[QW][2];
        Route rv[QW][2];
#pragma unroll
        for (int q = 0; q < QW; ++q)
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int32_t j = lane + m * WAVE;
                dv[q][m] = INF;
                e1[q][m] = e2[q][m] = INF;
                rv[q][m] = Route{1.0, 0, -1};
                if (!okq[q]) continue;
                const int32_t c = cq[q];
                if (c >= 0) {
                    const size_t x = sidx<L>(g, n, c, j);
                    dv[q][m] = SD[x];
                    rv[q][m] = SRT[x];
                } else if (SPE_LM_FUSE) {   // removed target: its three neighbours (k_expand_removed's rule)
                    const int32_t r = -2 - c;
                    dv[q][m] = SD[sidx<L>(g, n, G.rnb[3 * r], j)];
                    e1[q][m] = SD[sidx<L>(g, n, G.rnb[3 * r + 1], j)];
                    e2[q][m] = SD[sidx<L>(g, n, G.rnb[3 * r + 2], j)];
                } else {   // removed target: k_expand_removed's entry (sign = margin flag)
                    const size_t x = sidx<L>(g, nr, -2 - c, j);
                    dv[q][m] = DX[x];
                    rv[q][m] = RTX[x];
                }
            }
#pragma unroll
        for (int q = 0; q < QW; ++q) {
            if (!(SPE_LM_FUSE && okq[q] && cq[q] < 0)) continue;   // wave-uniform
            const int32_t r = -2 - cq[q];
            const int32_t u0 = G.rnb[3 * r], u1 = G.rnb[3 * r + 1], u2 = G.rnb[3 * r + 2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int32_t j = lane + m * WAVE;
                const double d0 = dv[q][m], d1 = e1[q][m], d2 = e2[q][m];
                const double a0 = d0 + G.rw[3 * r], a1 = d1 + G.rw[3 * r + 1], a2 = d2 + G.rw[3 * r + 2];
                int32_t k = d0 < INF ? 0 : -1;
                double bd = d0 < INF ? a0 : INF, bu = d0;
                const bool t1 = (d1 < INF) & ((a1 < bd) | ((a1 == bd) & (d1 < bu)));   // (branch-free: lex_less3)
                k = t1 ? 1 : k;
                bd = t1 ? a1 : bd;
                bu = t1 ? d1 : bu;
                const bool t2 = (d2 < INF) & ((a2 < bd) | ((a2 == bd) & (d2 < bu)));
                k = t2 ? 2 : k;
                bd = t2 ? a2 : bd;
                bool tight = false;
                if (check && k >= 0) {
                    if (k != 0 && d0 < INF) tight |= near_tie(bd, a0, wmin, omax, hmax);
                    if (k != 1 && d1 < INF) tight |= near_tie(bd, a1, wmin, omax, hmax);
                    if (k != 2 && d2 < INF) tight |= near_tie(bd, a2, wmin, omax, hmax);
                }
                Route rt = Route{1.0, 0, -1};
                double d = INF;
                if (k >= 0) {
                    const Route rc = SRT[sidx<L>(g, n, k == 0 ? u0 : (k == 1 ? u1 : u2), j)];
                    rt.r = rc.r * G.ra[3 * r + k];
                    rt.h = rc.h + 1;
                    rt.f = (rc.h == 0) ? rorig[r] : rc.f;   // the neighbour is the lane's root itself
                    d = tight ? -bd : bd;
                }
                dv[q][m] = d;
                rv[q][m] = rt;
            }
        }
#pragma unroll
        for (int q = 0; q < QW; ++q) {
            if (!okq[q]) continue;
            const int32_t tt = wib + q * (BLOCK / WAVE);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                sD[lane + m * WAVE][tt] = dv[q][m];
                sR[lane + m * WAVE][tt] = rv[q][m];
            }
        }
        __syncthreads();
        for (int32_t p = threadIdx.x; p < L * TS; p += BLOCK) {   // 16 threads per lane row: one 128-B line of XD
            const int32_t j = p / TS, q = p - (p / TS) * TS, t = t0 + q;
            if (t < A) {
                const size_t o = (size_t)(g * L + j) * (size_t)AP + (size_t)t;
                XD[o] = sD[j][q];
                XRT[o] = sR[j][q];
            }
        }
        __syncthreads();   // the next item overwrites the tile
    }
}

#ifndef SPE_LM_XCD_BLOCKS
#define SPE_LM_XCD_BLOCKS 1   // k_rows_lm: XCD = eighth of the source blocks (1) or of the target tiles (0)
#endif
#ifndef SPE_LM_PRELOAD
#define SPE_LM_PRELOAD 1   // a wave loads its 16 sources' ids, leg ranges and first legs once per item
#endif
#ifndef SPE_LM_PRELEGS
#define SPE_LM_PRELEGS 4   // legs per source preloaded (4 or 8; A/B with KL: 8 x 4 / 4 x 4 / 8 x 2 / 4 x 2 -> 39.7 / 37.2 / 40.4 / 36.8 ms)
#endif
#ifndef SPE_LM_KL
#define SPE_LM_KL 2        // legs per batch of staged-value loads (78 VGPRs: 6 waves / SIMD)
#endif
__device__ __forceinline__ DLeg shfl_leg(const DLeg& x, int32_t src) {
    DLeg r;
    r.w = __shfl(x.w, src);
    r.ref = __shfl(x.ref, src);
    r.pad0 = 0;
    r.a = __shfl(x.a, src);
    r.hopinc = __shfl(x.hopinc, src);
    r.pad1 = 0;
    return r;
}

#ifndef SPE_LM_WPE
// waves per SIMD k_rows_lm is compiled for: 7 (72 VGPRs; its 22.9 KB of LDS per block
// allows 7 blocks per CU) -- the compiler's own choice was 6 (78 VGPRs); A/B round 6:
// rows 97.5-98.8 -> 90.0-91.1 ms per two C3 tables
#define SPE_LM_WPE 7
#endif
#define SPE_LM_ATTR __attribute__((amdgpu_waves_per_eu(SPE_LM_WPE)))
template <bool GEN, bool DELIVERY = false>
__global__ __launch_bounds__(BLOCK) SPE_LM_ATTR void k_rows_lm(int32_t blocks, int32_t sb0, const int32_t* __restrict__ srcv,
                                                   const SlotInfo* __restrict__ slots, DevGraph G, RowMode md, Table tb,
                                                   const int2* __restrict__ lrng, const DLeg* __restrict__ legs,
                                                   const double* __restrict__ XD, const Route* __restrict__ XRT,
                                                   double wmin, double omax, double hmax, int32_t exact,
                                                   uint8_t* __restrict__ sunsafe,
                                                   Deliv dv = Deliv{nullptr, nullptr, 0}) {
    constexpr int T = LM_T, KL = SPE_LM_KL;
    constexpr int SPS = WAVE / T;                          // sources per wave step
    constexpr int SPW = WAVE / (BLOCK / WAVE);             // sources per wave (16)
    static_assert(WAVE % T == 0 && BLOCK == 256 && SPW % SPS == 0, "SPS sources x T targets per wave step");
    __shared__ dvec2 sLR[T][WAVE + 1];
    __shared__ int32_t sN[T][WAVE + 1];
    __shared__ uint16_t sH[T][WAVE + 2];
    const int32_t lane = threadIdx.x & (WAVE - 1), wib = threadIdx.x >> 6;
    const int32_t half = lane / T, tl = lane % T;   // (half: the lane's source of the step)
    const int64_t AP = lm_stride(tb.A);
    const int32_t ntile = (tb.A + T - 1) / T;
    const int64_t items_all = (int64_t)ntile * blocks;
    (void)items_all;
    const bool xs = (gridDim.x & 7) == 0;
    const int32_t xcd = xs ? (int32_t)(blockIdx.x & 7) : 0;
    const int64_t nwg = xs ? (int64_t)(gridDim.x >> 3) : (int64_t)gridDim.x;
    const int64_t wg0 = xs ? (int64_t)(blockIdx.x >> 3) : (int64_t)blockIdx.x;
#if SPE_LM_XCD_BLOCKS
    // each XCD takes a contiguous eighth of the source BLOCKS and walks it target-tile-
    // major: a block's legs read the lanes of its own cluster of roots (lanes follow the
    // slot order), so one tile's lane segments an XCD needs (~1/8 of the lanes: ~1 MB on
    // C3) stay in its L2 while that XCD's blocks read them -- where eighths of the TILES
    // over all blocks needed every lane's segment per tile (8.4 MB per 4-MB L2)
    const int32_t xb0 = xs ? (int32_t)((int64_t)blocks * xcd / 8) : 0;
    const int32_t xnb = xs ? (int32_t)((int64_t)blocks * (xcd + 1) / 8) - xb0 : blocks;
    const int64_t lo = 0, hi = (int64_t)ntile * xnb;
    for (int64_t it = lo + wg0; it < hi; it += nwg) {   // workgroup-uniform
        const int32_t tile = (int32_t)(it / xnb), b = xb0 + (int32_t)(it - (int64_t)(it / xnb) * xnb);
#else
    // target-tile-major items in XCD-contiguous ranges: one XCD's blocks read the same
    // 32-target segments of the lane rows from its L2
    const int64_t lo = xs ? items_all * xcd / 8 : 0, hi = xs ? items_all * (xcd + 1) / 8 : items_all;
    for (int64_t it = lo + wg0; it < hi; it += nwg) {   // workgroup-uniform
        const int32_t tile = (int32_t)(it / blocks), b = (int32_t)(it - (int64_t)tile * blocks);
#endif
        const int32_t t = tile * T + tl;
        const bool tv = t < tb.A;
        const SlotInfo sv = slots[tv ? t : tb.A - 1];
#if SPE_LM_PRELOAD
        static_assert(SPW == 16, "lane = (source of the wave, leg) for the preload");
        // lane l: source l / 4 of this wave's 16, legs l % 4 and l % 4 + 4: one round trip
        // per item instead of one per step; the steps take them with shuffles
        const int32_t pi = b * WAVE + wib * SPW + (lane >> 2);
        const int32_t ps = srcv[pi];
        const int2 plr = lrng[pi];
        const int32_t pnl = ps >= 0 ? (plr.y & 0xFFFF) : 0;
        DLeg pl[2];
        pl[0] = pl[1] = DLeg{0.0, 0, 0, 1.0, -1, 0};
#pragma unroll
        for (int h = 0; h < SPE_LM_PRELEGS / 4; ++h)
            if ((lane & 3) + 4 * h < pnl) pl[h] = legs[plr.x + (lane & 3) + 4 * h];
#endif
        for (int32_t step = 0; step < SPW / SPS; ++step) {   // SPW sources per wave, SPS per step
            const int32_t sl = wib * SPW + step * SPS + half;
            const int32_t i = b * WAVE + sl;
#if SPE_LM_PRELOAD
            const int32_t qsrc = (step * SPS + half) * 4;   // the preload lanes of this lane's source
            const int32_t s = __shfl(ps, qsrc);
            int2 lr;
            lr.x = __shfl(plr.x, qsrc);
            lr.y = __shfl(plr.y, qsrc);
#else
            const int32_t s = srcv[i];
            const int2 lr = lrng[i];
#endif
            const int32_t nl = s >= 0 ? (lr.y & 0xFFFF) : 0;
            const bool chk = (lr.y >> 16) != 0 && !exact;
            int32_t nlmax = 0;
#pragma unroll
            for (int q = 0; q < SPS; ++q) nlmax = max(nlmax, __builtin_amdgcn_readlane(nl, q * T));
            const bool live = tv && s >= 0 && sv.t != s;
            double bo = INF, m2 = INF, wa = 1.0;
            bool tg = false;
            int32_t wref = -1, whi = -1;
            int32_t wk = 0;   // (DELIVERY) the winning leg
            (void)wk;
            for (int32_t k0 = 0; k0 < nlmax; k0 += KL) {   // wave-uniform
                DLeg d[KL];
                double x[KL];
#if SPE_LM_PRELOAD
                if (k0 + KL <= SPE_LM_PRELEGS) {   // wave-uniform: the preloaded legs
#pragma unroll
                    for (int k = 0; k < KL; ++k)
                        d[k] = shfl_leg(k0 + k < 4 ? pl[0] : pl[1], qsrc + ((k0 + k) & 3));
                } else
#endif
                {
#pragma unroll
                    for (int k = 0; k < KL; ++k)
                        if (k0 + k < nl) d[k] = legs[lr.x + k0 + k];   // (a half's lanes read one record)
                }
#pragma unroll
                for (int k = 0; k < KL; ++k) {
                    x[k] = INF;
                    if (live && k0 + k < nl) {
                        if (d[k].ref >= 0) x[k] = XD[(size_t)d[k].ref * (size_t)AP + (size_t)t];
                        else if (leg_direct_tc(d[k].ref) == sv.c) x[k] = 0.0;
                    }
                }
                // running best first leg (strict: the first of equal sums wins; a tie
                // flags the source anyway) and the lowest tie floor of the others
#pragma unroll
                for (int k = 0; k < KL; ++k) {
                    if (!(live && k0 + k < nl)) continue;
                    const bool tight = chk && __builtin_signbit(x[k]);
                    const double o = d[k].w + __builtin_fabs(x[k]);
                    if (!(o < INF)) continue;
                    const bool better = o < bo;
                    const double loser = better ? bo : o;
                    if (loser < INF) m2 = fmin(m2, tie_floor(loser, wmin, omax, hmax, exact));
                    bo = better ? o : bo;
                    tg = better ? tight : tg;
                    wref = better ? d[k].ref : wref;
                    wa = better ? d[k].a : wa;
                    whi = better ? d[k].hopinc : whi;
                    if constexpr (DELIVERY) wk = better ? k0 + k : wk;
                }
            }
            bool bad = false;
            Route rc = Route{1.0, 0, -1};
            if (bo < INF) {
                if (nl > 1) bad |= m2 <= bo;   // u* must beat the other first legs by more than rounding
                bad |= tg;
                if (wref >= 0) rc = XRT[(size_t)wref * (size_t)AP + (size_t)t];
            }
            double Lt = -1.0, R = -1.0;
            int32_t N = -1, H = 0;
            if (tv && s >= 0) {
                if (sv.t == s) {
                    if constexpr (GEN) self_entry(G, md, s, Lt, R, N, H);   // else k_rows_self
                } else if (bo < INF) {
                    double dd = bo;
                    Route rt = rc;
                    if (whi >= 0) {   // a prefix in front: its edges, its first hop
                        rt.r = wa * rt.r;
                        rt.h = rt.h + (whi >> 29);
                        rt.f = whi & 0x1FFFFFFF;
                    }
                    if (GEN && sv.kt >= 0) {   // a pruned pendant target: one edge past its anchor
                        dd = dd + sv.pw;
                        rt.r = rt.r * sv.pa;
                        rt.f = (rt.h == 0) ? sv.t : rt.f;
                        rt.h = rt.h + 1;
                    }
                    Lt = dd == 0 ? 1.0 : dd;   // shd-topology.c:1833-1837
                    R = rt.r;
                    N = rt.f;
                    H = rt.h;
                }
            }
            if constexpr (DELIVERY) {   // a leg with a prefix reading a root lane: an offset entry
                const bool off = tv && s >= 0 && sv.t != s && bo < INF && whi >= 0 && wref >= 0;
                deliv_push(dv, b, off && delivery_near_boundary(Lt, H), sl + b * WAVE, t, wref, lr.x + wk);
            }
            dvec2 e;
            e.x = Lt;
            e.y = R;
            sLR[tl][sl] = e;
            sN[tl][sl] = N;
            sH[tl][sl] = (uint16_t)(H > 65535 ? 65535 : H);
            const uint64_t bb = __ballot(bad);
            constexpr uint64_t HM = T == 64 ? ~0ull : ((1ull << T) - 1ull);
            if (tl == 0 && ((bb >> (T * half)) & HM)) sunsafe[i] = 1;
        }
        __syncthreads();
        for (int32_t p = threadIdx.x; p < T * WAVE; p += BLOCK) {   // 64 threads per target: one 1-KB segment
            const int32_t q = p >> 6, sl = p & (WAVE - 1), tq = tile * T + q;
            if (tq < tb.A) {
                const size_t o = tidx(sb0 + b, tb.A, tq, sl);
                __builtin_nontemporal_store(sLR[q][sl], reinterpret_cast<dvec2*>(tb.lr + o));
                __builtin_nontemporal_store(sN[q][sl], tb.next + o);
                __builtin_nontemporal_store(sH[q][sl], tb.hops + o);
            }
        }
        __syncthreads();   // the next item overwrites the tile
    }
}

// The self entries (t == s) of the rows k_rows_derived<GEN = false> wrote: one thread
// per source slot of the launch's blocks (the source's own slot is its self target).
__global__ __launch_bounds__(BLOCK) void k_rows_self(int32_t blocks, int32_t sb0, int32_t slot0,
                                                     const int32_t* __restrict__ srcv, DevGraph G, RowMode md,
                                                     Table tb) {
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= blocks * WAVE) return;
    const int32_t s = srcv[i];
    const int32_t jt = slot0 + i;   // this source's slot = its self target
    if (s < 0 || jt >= tb.A) return;
    double Lt = -1.0, R = -1.0;
    int32_t N = -1, H = 0;
    self_entry(G, md, s, Lt, R, N, H);
    const size_t o = tidx(sb0 + i / WAVE, tb.A, jt, i % WAVE);
    tb.lr[o] = make_double2(Lt, R);
    tb.next[o] = N;
    tb.hops[o] = (uint16_t)(H > 65535 ? 65535 : H);
}

// spe_table_opts.exact_delivery: the path-order latency of every worklist record (one
// lane per record), as the source's own relaxation lane would have summed it
// (exact_sources = 1): from the winning leg's prefix -- fl(0 + w1), or fl(fl(0 + w1) +
// w2) for a two-edge leg, which is DLeg.w / the pendant edge bit for bit -- every tree
// entry from the root to the target's relaxation vertex as the relaxation offers it,
// fl(fl(L + iw[k]) + xw2[k]) (xw2 absent or 0: one add), then a removed target's last
// edge and a pendant target's edge.  The tree is the root lane's: its parent entries are
// walked back from the target (up to 64 kept and folded forward, longer paths re-walk per
// entry as aux_fold does).  Blocks over the cap are left alone: the host rebuilds them
// one lane per source.  Only the latency is stored; changed[b] counts block b's bit changes.
template <int L>
__global__ __launch_bounds__(BLOCK) void k_refold_delivery(int32_t n, int32_t blocks, int32_t sb0,
                                                           const SlotInfo* __restrict__ slots, DevGraph G, State st,
                                                           Table tb, const DLeg* __restrict__ legs,
                                                           const double2* __restrict__ rwa, Deliv dv,
                                                           uint32_t* __restrict__ changed) {
    constexpr int KMAX = 64;
    const int64_t nth = (int64_t)gridDim.x * BLOCK;
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    for (int32_t b = 0; b < blocks; ++b) {
        const uint32_t cnt = dv.cnt[b];
        if (cnt > (uint32_t)dv.cap) continue;
        uint32_t nch = 0;
        for (int64_t p = tid; p < (int64_t)cnt; p += nth) {
            const int4 rec = dv.work[(size_t)b * (size_t)dv.cap + (size_t)p];
            const int32_t i = rec.x, jt = rec.y, sl = rec.z;
            const SlotInfo si = slots[jt];
            const int32_t g = sl / L, j = sl % L;
            int32_t c = si.c;
            double last = 0.0;   // a removed target: the edge from the neighbour its row takes
            if (c < 0) {         // the best of its three neighbours (d, then d[u], then u), k_rows_sssp's rule
                const int32_t r = -2 - c;
                const double d0 = st.D[sidx<L>(g, n, G.rnb[3 * r], j)], d1 = st.D[sidx<L>(g, n, G.rnb[3 * r + 1], j)],
                             d2 = st.D[sidx<L>(g, n, G.rnb[3 * r + 2], j)];
                const double a0 = d0 + G.rw[3 * r], a1 = d1 + G.rw[3 * r + 1], a2 = d2 + G.rw[3 * r + 2];
                int32_t q = d0 < INF ? 0 : -1;
                double bd = d0 < INF ? a0 : INF, bu = d0;
                const bool t1 = (d1 < INF) & ((a1 < bd) | ((a1 == bd) & (d1 < bu)));
                q = t1 ? 1 : q;
                bd = t1 ? a1 : bd;
                bu = t1 ? d1 : bu;
                const bool t2 = (d2 < INF) & ((a2 < bd) | ((a2 == bd) & (d2 < bu)));
                q = t2 ? 2 : q;
                if (q < 0) continue;   // (unroutable entries are never flagged)
                c = G.rnb[3 * r + q];
                last = G.rw[3 * r + q];
            }
            int32_t ks[KMAX];
            int32_t nk = 0;
            for (int32_t x = c; nk <= n;) {   // (a tree path has fewer than n entries)
                const int32_t k = st.P[sidx<L>(g, n, x, j)];
                if (k < 0) break;             // the root
                if (nk < KMAX) ks[nk] = k;
                ++nk;
                x = G.icol[k];
            }
            double l = rec.w >= 0 ? legs[rec.w].w : rwa[i].x;
            for (int32_t q = nk - 1; q >= 0; --q) {
                int32_t k;
                if (q < KMAX) {
                    k = ks[q];
                } else {   // entry q (0 = the last one, into c)
                    int32_t x = c;
                    for (int32_t r = 0; r < q; ++r) x = G.icol[st.P[sidx<L>(g, n, x, j)]];
                    k = st.P[sidx<L>(g, n, x, j)];
                }
                l = l + G.iw[k];
                if (G.xw2) l = l + G.xw2[k];
            }
            if (si.c < 0) l = l + last;
            if (si.kt >= 0) l = l + si.pw;
            if (l == 0) l = 1;   // shd-topology.c:1833-1837
            double* e = reinterpret_cast<double*>(tb.lr + tidx(sb0 + (i >> 6), tb.A, jt, i & (WAVE - 1)));
            if (__double_as_longlong(*e) != __double_as_longlong(l)) {
                *e = l;
                ++nch;
            }
        }
        if (nch) atomicAdd(changed + b, nch);
    }
}

// Shared anchor trees: after a batch's relaxation over its roots, flag every root
// some of whose parent decisions a source offset could change.  A source s with
// offset o (its pendant edge, o <= omax) sums every path in the same order as its
// root but from o instead of 0; along a path of h edges each sum is within
// h u (o + d) of o + the exact sum (u = 2^-53), so a vertex whose parent's offer
// beats every other in-entry's offer alt by more than 4.5 H u (omax + alt) -- H
// bounding the edge count, alt / wmin + 3 -- keeps that parent, without a
// tie-break, for every such source; then every source's tree is the root's (DESIGN
// §4.1).  The test is per entry (alt - d - bound(alt) grows with alt, so the
// smallest competing offer fails it first), so in-lists split freely: one wave per
// (lane group, light vertex) or (lane group, 64-entry segment of a heavy vertex),
// four neighbour rows per round trip.
template <int L>
__global__ __launch_bounds__(BLOCK) void k_share_check(int32_t groups, int32_t n, const int32_t* __restrict__ srcv,
                                                       DevGraph G, State st, HeavyPlan hp, double wmin, double omax,
                                                       double hmax, uint8_t* __restrict__ unsafe) {
    constexpr int M = L > WAVE ? L / WAVE : 1;
    static_assert(L >= WAVE, "one lane group per wave");
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int64_t nw = ((int64_t)gridDim.x * BLOCK) >> 6;
    const int64_t light = (int64_t)groups * n;
    const int64_t items = light + (int64_t)groups * hp.nseg;
    for (int64_t it = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6; it < items; it += nw) {   // wave-uniform
        int32_t g, v, k0, k1;
        if (it < light) {
            g = (int32_t)(it / n);
            v = (int32_t)(it - (int64_t)g * n);
            k0 = G.iptr[v];
            k1 = G.iptr[v + 1];
            if (k1 - k0 > WAVE) continue;   // heavy: its segments below
        } else {
            const int64_t q = it - light;
            g = (int32_t)(q / hp.nseg);
            const int32_t sg = (int32_t)(q - (int64_t)g * hp.nseg);
            v = hp.seg_vertex[sg];
            k0 = hp.seg_begin[sg];
            k1 = min(k0 + WAVE, G.iptr[v + 1]);
        }
        double d[M];
        int32_t pk[M];
        bool act[M], any = false, bad[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int32_t j = lane + m * WAVE;
            const size_t i = sidx<L>(g, n, v, j);
            d[m] = st.D[i];
            pk[m] = st.P[i];
            act[m] = srcv[g * L + j] >= 0 && d[m] < INF && pk[m] != -1;   // (-1: the root itself)
            bad[m] = false;
            any |= act[m];
        }
        if (!__ballot(any)) continue;
        const int32_t k = k0 + lane;
        const bool ok = k < k1;
        const int4 pkk = ok ? G.ipack[k] : make_int4(0, 0, 0, 0);
        const double w_j = __hiloint2double(pkk.w, pkk.z);
        const double w2_j = (G.xw2 && ok) ? G.xw2[k] : 0.0;
        const int32_t cnt = k1 - k0;
        for (int32_t q = 0; q < cnt; q += 4) {
            double du[4][M];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int32_t u = __builtin_amdgcn_readlane(pkk.x, min(q + r, cnt - 1));
#pragma unroll
                for (int m = 0; m < M; ++m) du[r][m] = st.D[sidx<L>(g, n, u, lane + m * WAVE)];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (q + r >= cnt) break;
                const double w = sub_get_d<WAVE>(w_j, q + r), w2 = sub_get_d<WAVE>(w2_j, q + r);
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const double alt = (du[r][m] + w) + w2;   // the relaxation's fold (+ 0.0: one add)
                    if (!act[m] || k0 + q + r == pk[m] || !(alt < INF)) continue;
                    const double h = wmin > 0.0 ? fmin(hmax, alt / wmin + 3.0) : hmax;
                    bad[m] |= alt - d[m] <= 4.5 * h * 0x1p-53 * (omax + alt);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m)
            if (bad[m]) unsafe[(size_t)g * L + lane + m * WAVE] = 1;
    }
}

__global__ __launch_bounds__(BLOCK) void k_rows_direct(int32_t groups, int32_t sb0,
                                                       const int32_t* __restrict__ srcv,
                                                       const int32_t* __restrict__ slot_vertex, DevGraph G,
                                                       RowMode md, Table tb) {
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int64_t nwaves = ((int64_t)gridDim.x * BLOCK) >> 6;
    const int64_t items = (int64_t)groups * tb.A;
    for (int64_t it = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6; it < items; it += nwaves) {
        const int32_t g = (int32_t)(it / tb.A);
        const int32_t j = (int32_t)(it - (int64_t)g * tb.A);
        const int32_t t = slot_vertex[j];
        const int32_t s = srcv[g * WAVE + lane];
        double L = -1.0, R = -1.0;
        int32_t N = -1, H = 0;
        if (s >= 0) {
            if (t == s) self_entry(G, md, s, L, R, N, H);
            else direct_entry(G, s, t, L, R, N, H);
        }
        const size_t o = tidx(sb0 + g, tb.A, j, lane);
        tb.lr[o] = make_double2(L, R);
        tb.next[o] = N;
        tb.hops[o] = (uint16_t)H;
        if (tb.prev) tb.prev[o] = (H == 2) ? N : (H > 0 ? s : -1);
    }
}

// preferdirectpaths: every attached neighbour t of s takes the direct edge.
__global__ __launch_bounds__(BLOCK) void k_direct_overlay(int32_t groups, int32_t sb0,
                                                          const int32_t* __restrict__ srcv,
                                                          const int32_t* __restrict__ vertex_slot, DevGraph G,
                                                          Table tb) {
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= groups * WAVE) return;
    const int32_t g = i / WAVE, lane = i % WAVE;
    const int32_t s = srcv[i];
    if (s < 0) return;
    const double fs = G.vfac[s];
    for (int32_t k = G.dptr[s]; k < G.dptr[s + 1]; ++k) {
        const int32_t t = G.dcol[k];
        const int32_t j = vertex_slot[t];
        if (j < 0) continue;
        const double ft = G.vfac[t];
        double r = 1.0;
        if (has_attr(fs)) r *= fs;
        if (has_attr(ft)) r *= ft;
        r *= G.darep[k];
        const size_t o = tidx(sb0 + g, tb.A, j, lane);
        tb.lr[o] = make_double2(0.0 + G.dwrep[k], r);
        tb.next[o] = t;
        tb.hops[o] = 1;
        if (tb.prev) tb.prev[o] = s;
    }
}

