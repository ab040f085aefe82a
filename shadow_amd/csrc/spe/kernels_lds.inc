// kernels_lds.inc -- part of spe.hip (one translation unit; included inside its
// anonymous namespace).  LDS engine (k_sssp_lds), owner replay, lookups, table check, min latency.

// ------------------------------------------------------------------------
// LDS engine: one workgroup per source row with the row's relaxation state
// resident in LDS.  For graphs up to 10,240 relaxation vertices (Shadow's own
// topologies, C2) this replaces the 64-lane HBM-resident batch relaxation.
// Per source row:
//   1. push Bellman-Ford over a changed-vertex bitset: LDS 64-bit atomic min on
//      the distance bits (non-negative doubles order as integers); a wave takes
//      64 vertices and spreads their out-edges over its lanes (wave_expand), so
//      a round costs one global round trip per 64 edges, not one per edge;
//   2. canonical parent = argmin (d[u], u) over {u : fl(d[u] + w) == d[v]},
//      in-edges spread over lanes the same way, per-vertex argmin in LDS;
//   3. latencies of every target (d is final);
//   4. top-down over the parent tree by hop level, entirely in LDS: every
//      thread keeps its vertices' parent and parent-edge factor in registers and
//      a level settles each vertex whose parent settled in the previous one:
//      hops, the path-order reliability fold r(v) = r(parent) * (1 - p_e) and
//      the first hop, each computed once from the parent's final values;
//   5. reliability / next hop / hops of every target into the SB64 table.
// Distances are the least fixpoint of d[v] = min fl(d[u] + w), as in the batch
// engine, so rows are bit-identical (tests/test_gpu_lds.py).
constexpr int LDS_T = 1024;                 // threads per workgroup (16 waves)
constexpr int LDS_WAVES = LDS_T / WAVE;
constexpr int LDS_MAX_BYTES = 160 * 1024 - 1024;   // dynamic share; the rest covers static __shared__
constexpr int LDS_WL = 256;                 // per-wave marked-vertex list of the push pass
#ifndef LDS_WIN_N
#define LDS_WIN_N 3
#endif
constexpr int LDS_WIN = LDS_WIN_N;          // 64-edge windows per global round trip of the push pass
constexpr int LDS_CAND_BYTES = LDS_WAVES * (LDS_WL * 4 + LDS_WIN * WAVE);   // push lists + owner maps (H space)

__host__ __device__ constexpr size_t lds_align(size_t b) { return (b + 15) & ~(size_t)15; }
// D f64 | X i32 (out-row starts, then parent entry) | H u16 / argmin scratch | 2 bitsets
__host__ __device__ constexpr size_t lds_hs_bytes(int32_t nc) {
    return lds_align((size_t)nc * 2) > (size_t)LDS_CAND_BYTES ? lds_align((size_t)nc * 2) : (size_t)LDS_CAND_BYTES;
}
__host__ __device__ constexpr size_t lds_bytes(int32_t nc) {
    return lds_align((size_t)nc * 8) + lds_align((size_t)nc * 4) + lds_hs_bytes(nc) +
           2 * lds_align((size_t)((nc + 31) / 32) * 4);
}

// per-workgroup global scratch: the parent entries, kept for pass 5's rare
// path walks once the LDS parent array holds first hops
struct LdsScratch {
    int32_t* par;       // [grid][nc] in-CSR entry of each vertex's parent edge
};

// vertices per thread of the tree pass (registers): the LDS engine takes graphs
// of at most LDS_VPT * LDS_T = 10,240 relaxation vertices (C2's 9,998 fit; the
// register budget of 4 waves per SIMD leaves no room for 11)
constexpr int LDS_VPT = 10;

__device__ __forceinline__ int32_t par_vertex(const DevGraph& G, int32_t k) { return G.icol[k]; }

// Inclusive prefix sum over the wave in DPP (row shifts, then the two row
// broadcasts of the GFX9 DPP set): six VALU ops, where a shuffle-based scan is
// six dependent ds_bpermute round trips through the LDS crossbar.
__device__ __forceinline__ int32_t wave_incl_scan(int32_t v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);    // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);    // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);    // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);    // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

// Spread the edges of up to 64 owner lanes (lane l owns `deg` consecutive
// items) over the wave's lanes, 64 at a time.  body(ok, o, off) runs with the
// whole wave (so it may shuffle): item `off` of owner lane `o`, ok = a real item.
template <typename F>
__device__ __forceinline__ void wave_expand(int32_t lane, int32_t deg, F&& body) {
    const int32_t incl = wave_incl_scan(deg);
    const int32_t total = __builtin_amdgcn_readlane(incl, WAVE - 1);
    const int32_t excl = incl - deg;
    for (int32_t base = 0; base < total; base += WAVE) {
        const int32_t e = base + lane;
        int32_t o = 0;
#pragma unroll
        for (int step = WAVE / 2; step; step >>= 1) {
            const int32_t y = __shfl(incl, o + step - 1);
            if (y <= e) o += step;
        }
        const int32_t off = e - __shfl(excl, o);
        body(e < total, o, off, base, excl, incl);
    }
}

// Workgroup-wide OR with ONE barrier (__syncthreads_or costs three): call ix
// ORs into flag[ix % 3] and thread 0 clears flag[(ix + 2) % 3], which every
// thread read before this call's barrier and nobody writes before call ix + 2.
// ix must be workgroup-uniform and increase by one per call; flags start zero.
__device__ __forceinline__ bool wg_any(bool p, uint32_t& ix, int32_t* flag) {
    const uint32_t k = ix % 3u;
    if (__ballot(p) && (threadIdx.x & (WAVE - 1)) == 0) flag[k] = 1;
    __syncthreads();
    const bool r = flag[k] != 0;
    if (threadIdx.x == 0) flag[(k + 2u) % 3u] = 0;
    ++ix;
    return r;
}

__global__ __launch_bounds__(LDS_T) void k_sssp_lds(int32_t slot0, int32_t slot1, const SlotInfo* __restrict__ slots,
                                                     int32_t blk0, DevGraph G, RowMode md, Table tb, LdsScratch sc_,
                                                     unsigned long long* __restrict__ dbg) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int32_t nc = G.n;
    const int32_t nw = (nc + 31) / 32;
    double* D = reinterpret_cast<double*>(smem);
    unsigned long long* Db = reinterpret_cast<unsigned long long*>(smem);
    int32_t* X = reinterpret_cast<int32_t*>(smem + lds_align((size_t)nc * 8));
    unsigned char* hs = smem + lds_align((size_t)nc * 8) + lds_align((size_t)nc * 4);
    uint16_t* H = reinterpret_cast<uint16_t*>(hs);
    uint32_t* F0 = reinterpret_cast<uint32_t*>(hs + lds_hs_bytes(nc));
    uint32_t* F1 = F0 + lds_align((size_t)nw * 4) / 4;
    // after the latency pass the distance space holds the reliability fold and X
    // (parent, first hop); the parent entries move to Xg
    double* Rl = D;
    __shared__ int32_t s_any[3];
    uint32_t syncix = 0;
    const int32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if (tid < 3) s_any[tid] = 0;   // (the first slot's init barrier publishes it)
    const unsigned long long INF_BITS = 0x7FF0000000000000ull;
    const int32_t oend = G.optr[nc];
    // Workgroups are dealt round-robin over the 8 XCDs; give the workgroups of
    // one XCD consecutive slots so the partial 512-B SB64 segments each row
    // writes meet in the same L2 before write-back.
    const int32_t gx = gridDim.x;
    const int32_t bx = (gx % 8 == 0) ? (blockIdx.x % 8) * (gx / 8) + blockIdx.x / 8 : blockIdx.x;
    int32_t* Xg = sc_.par + (size_t)blockIdx.x * nc;
    for (int32_t slot = slot0 + bx; slot < slot1; slot += gx) {
        const int32_t s = slots[slot].t;
        unsigned long long tph = dbg && tid == 0 ? wall_clock64() : 0, nround = 0, nlev = 0;
#define LDS_PHASE(i)                                                        \
    if (dbg && tid == 0) {                                                  \
        const unsigned long long now = wall_clock64();                      \
        atomicAdd(&dbg[i], now - tph);                                      \
        tph = now;                                                          \
    }
        const int32_t sc = G.core_id[s];
        const int32_t seed = sc >= 0 ? sc : G.anchor_core[s];
        for (int32_t v = tid; v < nc; v += LDS_T) {
            Db[v] = INF_BITS;
            X[v] = G.optr[v];
        }
        for (int32_t w = tid; w < nw; w += LDS_T) {
            F0[w] = 0;
            F1[w] = 0;
        }
        __syncthreads();
        if (tid == 0) {
            // pruned pendant source: its first step s -> anchor is fixed (see k_init_state)
            D[seed] = sc >= 0 ? 0.0 : 0.0 + G.fiw[G.fiptr[s]];
            F0[seed >> 5] = 1u << (seed & 31);
        }
        __syncthreads();
        LDS_PHASE(0)
        // 1. push relaxation to the fixpoint.  Each wave reads 64 bitset words at
        // once (words wave, wave+16, ...), lists their marked vertices (up to
        // 256), then spreads the listed vertices' out-edges over its lanes, two
        // 64-edge windows per global round trip.
        uint32_t* cur = F0;
        uint32_t* nxt = F1;
        int32_t* wl = reinterpret_cast<int32_t*>(hs) + wave * LDS_WL;   // H space is idle here
        uint8_t* om = hs + LDS_WAVES * LDS_WL * 4 + wave * LDS_WIN * WAVE;
        for (;;) {
            bool any = false;
            int32_t cnt = 0;   // wave-uniform list length
            unsigned long long tfl = 0;
            auto flush = [&]() {
                const unsigned long long tf0 = (dbg && tid == 0) ? wall_clock64() : 0;
                for (int32_t lb = 0; lb < cnt; lb += WAVE) {
                const int32_t v = lb + lane < cnt ? wl[lb + lane] : -1;
                int32_t k0 = 0, deg = 0;
                double dv = 0.0;
                if (v >= 0) {
                    k0 = X[v];
                    deg = (v + 1 < nc ? X[v + 1] : oend) - k0;
                    dv = D[v];
                }
                const int32_t incl = wave_incl_scan(deg);
                const int32_t total = __builtin_amdgcn_readlane(incl, WAVE - 1);
                const int32_t excl = incl - deg;
                for (int32_t base = 0; base < total; base += LDS_WIN * WAVE) {
                    int32_t x[LDS_WIN];
                    double cand[LDS_WIN], du[LDS_WIN];
                    bool ok[LDS_WIN];
                    // owner map of this window: each lane stamps its own edges
                    for (int32_t i = max(excl, base), ie = min(incl, base + LDS_WIN * WAVE); i < ie; ++i)
                        om[i - base] = (uint8_t)lane;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                    for (int h = 0; h < LDS_WIN; ++h) {
                        const int32_t e = base + h * WAVE + lane;
                        const int32_t o = e < total ? om[e - base] : 0;
                        ok[h] = e < total;
                        // unconditional loads (index clamped): every window's edges
                        // are in flight together, one wait for all of them
                        const int32_t kr = __shfl(k0, o) + e - __shfl(excl, o);
                        const int32_t k = ok[h] ? kr : 0;
                        du[h] = __shfl(dv, o);
                        x[h] = G.ocol[k];
                        cand[h] = G.ow[k];
                    }
#pragma unroll
                    for (int h = 0; h < LDS_WIN; ++h) cand[h] += du[h];
#pragma unroll
                    for (int h = 0; h < LDS_WIN; ++h) {
                        if (!ok[h]) continue;
                        const unsigned long long cb = (unsigned long long)__double_as_longlong(cand[h]);
                        if (cb < atomicMin(&Db[x[h]], cb)) {
                            atomicOr(&nxt[x[h] >> 5], 1u << (x[h] & 31));
                            any = true;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();   // owner map reads done before the next stamps
                }
                }
                cnt = 0;
                if (dbg && tid == 0) tfl += wall_clock64() - tf0;
            };
            for (int32_t w0 = wave; w0 < nw; w0 += LDS_WAVES * WAVE) {
                const int32_t wi = w0 + lane * LDS_WAVES;
                uint32_t W = wi < nw ? cur[wi] : 0u;
                uint64_t pend = __ballot(W != 0);
                if (!pend) continue;
                if (W) cur[wi] = 0;   // consumed (each word belongs to one wave)
                while (pend) {
                    const bool mine = (pend >> lane) & 1ull;
                    const int32_t c = mine ? __popc(W) : 0;
                    const int32_t incl = wave_incl_scan(c);
                    const bool fit = mine && incl <= LDS_WL - cnt;   // a prefix of the pending lanes
                    const uint64_t fm = __ballot(fit);
                    if (!fm) {   // list full: process it, then retry
                        flush();
                        continue;
                    }
                    if (fit) {
                        int32_t pos = cnt + incl - c;
                        for (uint32_t x = W; x; x &= x - 1) wl[pos++] = wi * 32 + __builtin_ctz(x);
                    }
                    cnt += __builtin_amdgcn_readlane(incl, 63 - __builtin_clzll(fm));
                    pend &= ~fm;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (pend) flush();
                }
            }
            if (cnt) flush();
            ++nround;
            const unsigned long long tb0 = (dbg && tid == 0) ? wall_clock64() : 0;
            const bool more = wg_any(any, syncix, s_any);
            if (dbg && tid == 0) {
                atomicAdd(&dbg[11], tfl);
                atomicAdd(&dbg[12], wall_clock64() - tb0);
            }
            if (!more) break;
            uint32_t* tmp = cur;
            cur = nxt;
            nxt = tmp;
        }
        LDS_PHASE(1)
#ifdef SPE_LDS_PUSH_ONLY   // timing build (tools/gpu_pushonly.sh): the push alone, no rows
        continue;
#endif
        // 2. canonical parents: X[v] = in-CSR entry, -1 none (source), -2 pendant seed.
        // One flat pass over the in-CSR registers every valid candidate
        // (fl(d[u] + w) == d[v] > d[u]); a vertex with exactly one takes it, a
        // vertex with several (exact ties) rescans its in-list for argmin (d[u], u).
        // (Recording the push's improving edge and validating it instead was
        // measured slower: Gauss-Seidel reads make a vertex re-offer the value it
        // already gave, so equal offers cannot tell ties apart.)
        // Candidate counts are u16 halves of the (idle) H space, bumped by
        // non-returning LDS adds: a returning atomic per candidate would put an
        // LDS round trip on every valid in-entry.
        uint32_t* CNT = reinterpret_cast<uint32_t*>(hs);
        for (int32_t v = tid; v < nc; v += LDS_T) X[v] = (v == seed) ? (sc >= 0 ? -1 : -2) : -1;
        for (int32_t w = tid; w < (nc + 1) / 2; w += LDS_T) CNT[w] = 0;
        __syncthreads();
        {
            const int32_t m_rel = G.iptr[nc];
#ifndef LDS_PARENT_U
#define LDS_PARENT_U 8
#endif
            constexpr int U = LDS_PARENT_U;
            for (int32_t e0 = tid; e0 < m_rel; e0 += U * LDS_T) {
                int32_t u[U], v[U];
                double w[U];
#pragma unroll
                for (int q = 0; q < U; ++q) {   // unconditional (clamped) loads: all U in flight
                    const int32_t e = min(e0 + q * LDS_T, m_rel - 1);
                    const uint32_t uv = G.ipair[e];   // 12 B per entry instead of 16
                    u[q] = (int32_t)(uv & 0xFFFFu);
                    v[q] = (int32_t)(uv >> 16);
                    w[q] = G.iw[e];
                }
#pragma unroll
                for (int q = 0; q < U; ++q)
                    if (e0 + q * LDS_T >= m_rel) u[q] = -1;
#pragma unroll
                for (int q = 0; q < U; ++q) {
                    if (u[q] < 0 || v[q] == seed) continue;
                    const double du = D[u[q]], dv = D[v[q]];
                    const double alt = du + w[q];
                    if (du < INF && alt == dv && alt > du) {
                        X[v[q]] = e0 + q * LDS_T;   // the only writer unless the count says tie
                        atomicAdd(&CNT[v[q] >> 1], 1u << ((v[q] & 1) * 16));
                    }
                }
            }
        }
        __syncthreads();
        for (int32_t v = tid; v < nc; v += LDS_T) {   // exact ties: canonical argmin (d[u], u)
            if (((CNT[v >> 1] >> ((v & 1) * 16)) & 0xFFFFu) < 2u) continue;
            const double dv = D[v];
            double bdu = INF;
            int32_t bu = -1, bk = -1;
            for (int32_t k = G.iptr[v]; k < G.iptr[v + 1]; ++k) {
                const int32_t u = G.icol[k];
                const double du = D[u];
                if (!(du < INF)) continue;
                const double alt = du + G.iw[k];
                // branch-free (lex_less2, kernels_relax.inc:211-223)
                const bool better = (alt == dv) & (alt > du) & lex_less2(du, u, bdu, bu);
                bdu = better ? du : bdu;
                bu = better ? u : bu;
                bk = better ? k : bk;
            }
            X[v] = bk;
        }
        __syncthreads();
        LDS_PHASE(2)
        // 3. latencies (distances are final); unreachable targets complete here
        const int32_t sb_local = slot / WAVE - blk0, lane_s = slot % WAVE;
        // Targets go UR at a time: their slot records (and in pass 5 the next-hop
        // ids) are loaded together, one memory round trip per UR targets.
        constexpr int UR = 4;
        for (int32_t j0 = tid; j0 < tb.A; j0 += UR * LDS_T) {
        SlotInfo sv[UR];
#pragma unroll
        for (int q = 0; q < UR; ++q) sv[q] = slots[min(j0 + q * LDS_T, tb.A - 1)];
#pragma unroll
        for (int q = 0; q < UR; ++q) {
            const int32_t j = j0 + q * LDS_T;
            const SlotInfo& si = sv[q];
            if (j >= tb.A || si.t == s) continue;
            const size_t o = tidx(sb_local, tb.A, j, lane_s);
            if (Db[si.c] == INF_BITS) {
                tb.lr[o] = make_double2(-1.0, -1.0);
                tb.next[o] = -1;
                tb.hops[o] = 0;
                if (tb.prev) tb.prev[o] = -1;
            } else if (!md.multi_rep) {
                double l = si.kt >= 0 ? D[si.c] + si.pw : D[si.c];
                if (l == 0) l = 1;   // shd-topology.c:1833-1837
                tb.lr[o].x = l;
            }
        }
        }
        __syncthreads();
        LDS_PHASE(3)
        // 4. hops, first hop and the reliability fold over the parent tree.
        // Thread-owned vertices v = tid + i * LDS_T keep (parent, 1 - p of the
        // parent edge) in registers (relaxation-vertex ids: nc <= LDS_VPT * LDS_T
        // < 2^16).  Hops and first hop are integers, so pointer jumping gets them
        // exactly in ~log2(depth) rounds: W[v] = (jump << 16) | dist, "jump is
        // dist hops above v", ends at the terminal vertices (the seed's children
        // for a core source, the anchor seed for a pruned pendant source), whose
        // jump is themselves; then jump = the first hop and hops = dist + 1.  The
        // reliability product must fold in path order, so it runs top-down, one
        // barrier per hop level, each vertex at the level known from its hops.
        // X becomes W, then PF: first hop (high 16 bits, 0xFFFF = none) | parent.
        uint32_t* PF = reinterpret_cast<uint32_t*>(X);
        __shared__ uint32_t s_maxh;
        double pa[LDS_VPT];
        uint16_t par[LDS_VPT];
        uint32_t w[LDS_VPT];
        uint32_t todo = 0;
        const int32_t tpar = sc >= 0 ? seed : -1;   // a parent that makes its child terminal
#pragma unroll
        for (int i = 0; i < LDS_VPT; ++i) {
            const int32_t v = tid + i * LDS_T;
            int32_t k = -1;
            if (v < nc) {
                k = X[v];
                Xg[v] = k;
            }
            pa[i] = (double)k;   // the parent entry for now; its factor is loaded below
            par[i] = k >= 0 ? (uint16_t)par_vertex(G, k) : (uint16_t)0;
            if (k >= 0) todo |= 1u << i;
            w[i] = k < 0 ? ((v == seed && sc < 0) ? ((uint32_t)seed << 16) : 0xFFFFFFFFu)
                         : ((int32_t)par[i] == tpar ? ((uint32_t)v << 16) : (((uint32_t)par[i] << 16) | 1u));
        }
        if (tid == 0) s_maxh = 0;
        __syncthreads();   // every X read before W overwrites it
        uint32_t act = 0;
#pragma unroll
        for (int i = 0; i < LDS_VPT; ++i) {
            const int32_t v = tid + i * LDS_T;
            if (v < nc) PF[v] = w[i];
            if (((todo >> i) & 1u) && (w[i] >> 16) != (uint32_t)v) act |= 1u << i;
        }
        __syncthreads();
        LDS_PHASE(4)
        // parent-edge factors: requested here, first needed by the level pass, so
        // their latency hides behind the pointer jumping (unconditional, clamped)
#pragma unroll
        for (int i = 0; i < LDS_VPT; ++i) pa[i] = G.ia[((todo >> i) & 1u) ? (int32_t)pa[i] : 0];
        {
            auto wload = [&](uint32_t j) -> uint32_t {
                return __hip_atomic_load(PF + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            // in place and asynchronous: any (jump, dist) pair read is valid, so
            // composing with a newer one only shortens the chain
            for (;;) {
                uint32_t wj[LDS_VPT];
#pragma unroll
                for (int i = 0; i < LDS_VPT; ++i) wj[i] = ((act >> i) & 1u) ? wload(w[i] >> 16) : 0u;
#pragma unroll
                for (int i = 0; i < LDS_VPT; ++i) {
                    if (!((act >> i) & 1u)) continue;
                    const uint32_t j = w[i] >> 16;
                    if ((wj[i] >> 16) == j) {   // j is terminal: done
                        act &= ~(1u << i);
                    } else {
                        w[i] = (wj[i] & 0xFFFF0000u) | ((w[i] + wj[i]) & 0xFFFFu);
                        __hip_atomic_store(PF + tid + i * LDS_T, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                if (!wg_any(act != 0, syncix, s_any)) break;
            }
            uint32_t hmax = 0;
#pragma unroll
            for (int i = 0; i < LDS_VPT; ++i) {
                if (!((todo >> i) & 1u)) continue;
                const int32_t v = tid + i * LDS_T;
                const uint32_t h = (w[i] & 0xFFFFu) + 1u;
                H[v] = (uint16_t)h;
                PF[v] = (w[i] & 0xFFFF0000u) | par[i];
                w[i] = h;
                hmax = max(hmax, h);
            }
#pragma unroll
            for (int i = 0; i < LDS_VPT; ++i) {   // no parent: the seed or unreachable
                const int32_t v = tid + i * LDS_T;
                if (v < nc && !((todo >> i) & 1u)) {
                    H[v] = v == seed ? (sc >= 0 ? 0 : 1) : 0xFFFF;
                    PF[v] = (v == seed && sc < 0) ? (((uint32_t)seed << 16) | 0xFFFFu) : 0xFFFFFFFFu;
                }
            }
            for (int d = 1; d < WAVE; d <<= 1) hmax = max(hmax, (uint32_t)__shfl_xor((int)hmax, d));
            if (lane == 0 && hmax) atomicMax(&s_maxh, hmax);
            if (tid == 0) {
                const double fs = G.vfac[s];
                const double r0 = has_attr(fs) ? 1.0 * fs : 1.0;   // shd-topology.c:1428-1430
                Rl[seed] = sc >= 0 ? r0 : r0 * G.fia[G.fiptr[s]];
            }
            __syncthreads();
            const uint32_t levels = s_maxh;
            for (uint32_t l = 1; l <= levels; ++l) {
#pragma unroll
                for (int i = 0; i < LDS_VPT; ++i)
                    if (((todo >> i) & 1u) && w[i] == l) Rl[tid + i * LDS_T] = Rl[par[i]] * pa[i];
                __syncthreads();
            }
            nlev = levels;
        }
        LDS_PHASE(5)
        // 5. reliability, next hop, hops (+ latency re-fold for multigraphs)
        for (int32_t j0 = tid; j0 < tb.A; j0 += UR * LDS_T) {
        SlotInfo sv[UR];
        int32_t nh[UR];
#pragma unroll
        for (int q = 0; q < UR; ++q) sv[q] = slots[min(j0 + q * LDS_T, tb.A - 1)];
#pragma unroll
        for (int q = 0; q < UR; ++q) {
            const uint32_t fc = PF[sv[q].c] >> 16;
            nh[q] = G.corev[fc == 0xFFFFu ? 0u : fc];
        }
#pragma unroll
        for (int q = 0; q < UR; ++q) {
            const int32_t j = j0 + q * LDS_T;
            if (j >= tb.A) continue;
            const SlotInfo& si = sv[q];
            const int32_t t = si.t;
            const size_t o = tidx(sb_local, tb.A, j, lane_s);
            if (t == s) {
                double Lt = -1.0, R = -1.0;
                int32_t N = -1, Hh = 0;
                self_entry(G, md, s, Lt, R, N, Hh);
                tb.lr[o] = make_double2(Lt, R);
                tb.next[o] = N;
                tb.hops[o] = (uint16_t)Hh;
                if (tb.prev) tb.prev[o] = (Hh == 2) ? N : (Hh > 0 ? s : -1);
                continue;
            }
            const int32_t c = si.c, kt = si.kt;
            const uint16_t hc = H[c];
            if (hc == 0xFFFF) continue;   // unreachable: written in pass 3
            const int32_t Hh = hc + (kt >= 0 ? 1 : 0);
            double R;
            if (si.fast) {   // t's vertex factor absent or 1.0
                R = Rl[c] * si.pa;   // pa = 1.0 for relaxation vertices (exact)
            } else {   // ((1 * fs) * ft) * a1 * a2 ... : the target factor comes second
                const double ft = G.vfac[t];
                const double fs = G.vfac[s];
                double r = 1.0;
                if (has_attr(fs)) r *= fs;
                r *= ft;
                for (int32_t i = 1; i <= Hh; ++i) {
                    int32_t back = Hh - i;
                    double ea;
                    if (kt >= 0 && back == 0) {
                        ea = si.pa;
                    } else {
                        int32_t x = c;
                        if (kt >= 0) back -= 1;
                        for (int32_t q = 0; q < back; ++q) x = par_vertex(G, Xg[x]);
                        ea = Xg[x] >= 0 ? G.ia[Xg[x]] : G.fia[G.fiptr[s]];
                    }
                    r *= ea;
                }
                R = r;
            }
            if (md.multi_rep) {   // path-order re-fold of the get_eid latencies
                double l = 0.0;
                for (int32_t i = 1; i <= Hh; ++i) {
                    int32_t back = Hh - i;
                    double ew;
                    if (kt >= 0 && back == 0) {
                        ew = G.fiwrep[kt];
                    } else {
                        int32_t x = c;
                        if (kt >= 0) back -= 1;
                        for (int32_t q = 0; q < back; ++q) x = par_vertex(G, Xg[x]);
                        ew = Xg[x] >= 0 ? G.iwrep[Xg[x]] : G.fiwrep[G.fiptr[s]];
                    }
                    l += ew;
                }
                if (l == 0) l = 1;
                tb.lr[o].x = l;
            }
            tb.lr[o].y = R;
            const uint32_t fc = PF[c] >> 16;
            tb.next[o] = kt >= 0 && hc == 0 ? t : (fc == 0xFFFFu ? -1 : nh[q]);
            tb.hops[o] = (uint16_t)Hh;
            if (tb.prev) tb.prev[o] = kt >= 0 ? G.corev[c] : (Xg[c] >= 0 ? G.corev[par_vertex(G, Xg[c])] : s);
        }
        }
        __syncthreads();
        LDS_PHASE(6)
        if (dbg && tid == 0) {
            atomicAdd(&dbg[8], nround);
            atomicAdd(&dbg[9], nlev);
            atomicAdd(&dbg[10], 1ull);
        }
    }
#undef LDS_PHASE
}

// Owner replay (compat with the reference's first-writer-wins path cache,
// _topology_shouldStorePath shd-topology.c:1292-1321 + the either-direction
// lookup of _topology_getPathEntry :1952-2034): for each unordered slot pair,
// the source that ran first stores its path if it is not DIRECT and routable,
// the second stores only if the first did not; a non-DIRECT query answers its
// own stored path, else the reverse one (same latency / reliability / hops; next
// hop = the vertex before the querier on the owner's path when undirected, -1
// when directed), else fails.  One lane per pair (i < j): lane = i of a
// 64-slot block, wave = (block, j).
__device__ __forceinline__ bool has_edge(const DevGraph& G, int32_t a, int32_t b) {
    int32_t lo = G.dptr[a], hi = G.dptr[a + 1];
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (G.dcol[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo < G.dptr[a + 1] && G.dcol[lo] == b;
}

__global__ __launch_bounds__(BLOCK) void k_owner_replay(int32_t A, const int32_t* __restrict__ rank,
                                                        const int32_t* __restrict__ slot_vertex, DevGraph G,
                                                        RowMode md, Table tb) {
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int64_t nblk = (A + WAVE - 1) / WAVE;
    const int64_t items = nblk * A;
    const int64_t nwaves = ((int64_t)gridDim.x * BLOCK) >> 6;
    for (int64_t it = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6; it < items; it += nwaves) {
        const int32_t bi = (int32_t)(it / A);
        const int32_t j = (int32_t)(it - (int64_t)bi * A);
        const int32_t i = bi * WAVE + lane;
        if (i >= A || i >= j) continue;
        const int32_t vi = slot_vertex[i], vj = slot_vertex[j];
        const bool dij = md.prefer && has_edge(G, vi, vj);   // DIRECT, never cached
        const bool dji = md.prefer && has_edge(G, vj, vi);
        const size_t oij = tidx(bi, A, j, lane);
        const size_t oji = tidx(j / WAVE, A, i, j % WAVE);
        const bool i_first = rank[i] < rank[j];
        const size_t of = i_first ? oij : oji, oo = i_first ? oji : oij;
        const bool dfo = i_first ? dij : dji, dof = i_first ? dji : dij;
        const double2 ef = tb.lr[of], eo = tb.lr[oo];
        const double lf = ef.x, lo_ = eo.x;
        const bool sf = !dfo && lf > -1.0;                 // first runner stored (f, o)
        const bool so = !dof && lo_ > -1.0 && !sf;         // second stored (o, f)
        const double rf = ef.y, ro = eo.y;
        const uint16_t hf = tb.hops[of], ho = tb.hops[oo];
        const int32_t pf = tb.prev[of], po = tb.prev[oo];
        if (!dfo && !sf) {   // (f, o) answers the reverse path or fails
            tb.lr[of] = make_double2(so ? lo_ : -1.0, so ? ro : -1.0);
            tb.hops[of] = so ? ho : 0;
            tb.next[of] = (so && !md.directed) ? po : -1;
        }
        if (!dof && !so) {   // (o, f)
            tb.lr[oo] = make_double2(sf ? lf : -1.0, sf ? rf : -1.0);
            tb.hops[oo] = sf ? hf : 0;
            tb.next[oo] = (sf && !md.directed) ? pf : -1;
        }
    }
}


// Whole-table self-check (spe_table_check): one thread per SB64 entry (s, t),
// s != t.  Counters: [0] pairs, [1] unroutable, [2] bad values, [3] next hop not
// adjacent to s, [4] hop checks, [5] hop mismatches, [6] symmetry checks, [7]
// symmetry mismatches, [8] max relative asymmetry (f64 bits), [9] first bad pair
// (s << 32 | t, ~0 = none).  The checks are the per-target walk's consequences
// (shd-topology.c:1790-1849): the next hop is the path's second vertex, so it is
// adjacent to s, and on unique shortest paths hops(s, t) = 1 + hops(next, t);
// on an undirected graph lat(s, t) and lat(t, s) sum the same edges in opposite
// orders.
__device__ __forceinline__ void check_bad(unsigned long long* c, int32_t s, int32_t t) {
    atomicCAS(&c[9], ~0ull, ((unsigned long long)(uint32_t)s << 32) | (uint32_t)t);
}

__global__ __launch_bounds__(BLOCK) void k_table_check(int32_t A, const int32_t* __restrict__ slot_vertex,
                                                       const int32_t* __restrict__ vertex_slot, DevGraph G,
                                                       int32_t undirected, int32_t hop_rule, Table tb,
                                                       unsigned long long* __restrict__ c) {
    const int64_t total = (int64_t)((A + WAVE - 1) / WAVE) * A * WAVE;
    unsigned long long n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double worst = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLOCK) {
        const int32_t b = (int32_t)(i / ((int64_t)A * WAVE));
        const int64_t rem = i - (int64_t)b * A * WAVE;
        const int32_t ts = (int32_t)(rem / WAVE), ss = b * WAVE + (int32_t)(rem % WAVE);
        if (ss >= A || ss == ts) continue;
        ++n[0];
        const double2 e = tb.lr[i];
        if (!(e.x > -1.0)) {
            ++n[1];
            continue;
        }
        const int32_t sv = slot_vertex[ss], tv = slot_vertex[ts];
        const int32_t nx = tb.next[i];
        const int32_t h = tb.hops[i];
        bool bad = false;
        if (!(e.x > 0.0) || !(e.y > 0.0 && e.y <= 1.0) || h < 1 || nx < 0 || nx >= G.n_full) {
            ++n[2];
            bad = true;
        } else {
            if (!has_edge(G, sv, nx)) {
                ++n[3];
                bad = true;
            }
            const int32_t xs = vertex_slot[nx];
            if (hop_rule && xs >= 0 && nx != tv) {
                ++n[4];
                const int32_t h2 = tb.hops[tidx(xs / WAVE, A, ts, xs % WAVE)];
                if (h != 1 + h2) {
                    ++n[5];
                    bad = true;
                }
            }
            if (undirected) {
                ++n[6];
                const double2 r = tb.lr[tidx(ts / WAVE, A, ss, ts % WAVE)];
                const double dl = fabs(e.x - r.x) / e.x, dr = fabs(e.y - r.y) / e.y;
                const double d = fmax(dl, dr);
                worst = fmax(worst, d);
                if (!(d <= 1e-12)) {
                    ++n[7];
                    bad = true;
                }
            }
        }
        if (bad) check_bad(c, ss, ts);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        unsigned long long v = n[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & (WAVE - 1)) == 0 && v) atomicAdd(&c[k], v);
    }
    for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o));
    if ((threadIdx.x & (WAVE - 1)) == 0 && worst > 0.0) atomicMax(&c[8], (unsigned long long)__double_as_longlong(worst));
}

// Two tables over the same slots and blocks, entry by entry (spe_table_compare).
// Counters: [0] pairs, [1] routable in b, [2] route mismatches, [3] latency bits
// differ, [4] reliability bits differ, [5] beyond tolerance, [6] delivery flips
// (ceil(lat * 1e6), shd-worker.c:244), [7] / [8] max relative latency / reliability
// difference (f64 bits), [9] first bad pair (s << 32 | t).
__global__ __launch_bounds__(BLOCK) void k_table_compare(int32_t A, int32_t blk0, int64_t total, Table a, Table b,
                                                         double tol, unsigned long long* __restrict__ c) {
    unsigned long long n[7] = {0, 0, 0, 0, 0, 0, 0};
    double wl = 0.0, wr = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLOCK) {
        const int32_t blk = (int32_t)(i / ((int64_t)A * WAVE));
        const int64_t rem = i - (int64_t)blk * A * WAVE;
        const int32_t ts = (int32_t)(rem / WAVE), ss = (blk0 + blk) * WAVE + (int32_t)(rem % WAVE);
        if (ss >= A) continue;
        ++n[0];
        const double2 ea = a.lr[i], eb = b.lr[i];
        const bool oa = ea.x > -1.0, ob = eb.x > -1.0;
        n[1] += ob;
        bool bad = oa != ob || a.next[i] != b.next[i] || a.hops[i] != b.hops[i];
        n[2] += bad;
        if (oa && ob) {
            n[3] += __double_as_longlong(ea.x) != __double_as_longlong(eb.x);
            n[4] += __double_as_longlong(ea.y) != __double_as_longlong(eb.y);
            // bit-equal values are zero error (two reliabilities of 0 would give 0 / 0)
            const double dl = ea.x == eb.x ? 0.0 : fabs(ea.x - eb.x) / fabs(eb.x);
            const double dr = ea.y == eb.y ? 0.0 : fabs(ea.y - eb.y) / fabs(eb.y);
            wl = fmax(wl, dl);
            wr = fmax(wr, dr);
            const bool out = !(dl <= tol) || !(dr <= tol);
            n[5] += out;
            bad |= out;
            n[6] += ceil(ea.x * 1000000.0) != ceil(eb.x * 1000000.0);
        }
        if (bad) check_bad(c, ss, ts);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        unsigned long long v = n[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & (WAVE - 1)) == 0 && v) atomicAdd(&c[k], v);
    }
    for (int o = 32; o > 0; o >>= 1) {
        wl = fmax(wl, __shfl_xor(wl, o));
        wr = fmax(wr, __shfl_xor(wr, o));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {   // non-negative doubles order as integers
        if (wl > 0.0) atomicMax(&c[7], (unsigned long long)__double_as_longlong(wl));
        if (wr > 0.0) atomicMax(&c[8], (unsigned long long)__double_as_longlong(wr));
    }
}

// Per-block table digests (spe_table_digest, include/spe.h states the definition):
//   digest[b][f] = sum over s in block b (s < A), t in [0, A) of
//                  mix(bits_f(s, t) + km(s, t) * (2 f + 1)),  km = mix(s * A + t + 1),
// all on uint64 mod 2^64, mix = the splitmix64 finaliser.  The sum commutes, so the
// 64 bits do not depend on which wave adds what when.
//
// An HBM stream: a work item is (block, chunk of DG_TC targets), one wave per item,
// lane = source lane, one target per step -- the record load is the 1-KB SB64
// segment (16 B per lane), the next hops 256 B, the hop counts 128 B.  Every lane
// carries the four sums of its source; the item ends with a wave reduction (shuffles
// of the 32-bit halves) and one 64-bit atomic add per field into out[block][f].
// Lanes of the last block at or past A (padding: no source) load nothing and add 0.
// All pointers address block b0's first element; `mask` bit f = field f is wanted
// (a replica that holds only records: mask 3 costs only the record stream).
constexpr int32_t DG_TC = 128;

__device__ __forceinline__ unsigned long long dg_mix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(BLOCK) void k_table_digest(int32_t A, int32_t b0, int32_t nb,
                                                        const double2* __restrict__ lr,
                                                        const int32_t* __restrict__ nx,
                                                        const uint16_t* __restrict__ hp, uint32_t mask,
                                                        unsigned long long* __restrict__ out) {
    const int32_t lane = threadIdx.x & (WAVE - 1);
    const int32_t chunks = (A + DG_TC - 1) / DG_TC;
    const int64_t items = (int64_t)nb * chunks;
    const int64_t waves = (int64_t)gridDim.x * (BLOCK / WAVE);
    const bool want_lr = (mask & 3u) != 0, want_nx = (mask & 4u) != 0, want_hp = (mask & 8u) != 0;
    for (int64_t it = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE; it < items; it += waves) {
        const int32_t bl = (int32_t)(it / chunks);                     // wave-uniform
        const int32_t t0 = (int32_t)(it - (int64_t)bl * chunks) * DG_TC;
        const int32_t t1 = min(A, t0 + DG_TC);
        const int32_t s = (b0 + bl) * WAVE + lane;
        unsigned long long acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
        if (s < A) {
            unsigned long long key1 = (unsigned long long)s * (unsigned long long)A + (unsigned long long)t0 + 1ull;
            size_t o = tidx(bl, A, t0, lane);
#pragma unroll 4
            for (int32_t t = t0; t < t1; ++t, ++key1, o += WAVE) {
                const unsigned long long km = dg_mix(key1), k2 = km << 1;   // km once per pair
                if (want_lr) {
                    const double2 e = lr[o];
                    acc0 += dg_mix((unsigned long long)__double_as_longlong(e.x) + km);
                    acc1 += dg_mix((unsigned long long)__double_as_longlong(e.y) + km + k2);
                }
                if (want_nx) acc2 += dg_mix((unsigned long long)(uint32_t)nx[o] + km + k2 + k2);
                if (want_hp) acc3 += dg_mix((unsigned long long)hp[o] + km + k2 + k2 + k2);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            acc0 += __shfl_xor(acc0, off);
            acc1 += __shfl_xor(acc1, off);
            acc2 += __shfl_xor(acc2, off);
            acc3 += __shfl_xor(acc3, off);
        }
        if (lane == 0) {
            unsigned long long* d = out + (size_t)bl * 4;
            if (mask & 1u) atomicAdd(d + 0, acc0);
            if (mask & 2u) atomicAdd(d + 1, acc1);
            if (want_nx) atomicAdd(d + 2, acc2);
            if (want_hp) atomicAdd(d + 3, acc3);
        }
    }
}

// A system-scope release: the device caches write back what the table's kernels
// wrote, so host loads through a large-BAR mapping see it (table_host_reads).
__global__ void k_release_system() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, ""); }

template <int NT>
__global__ __launch_bounds__(BLOCK) void k_lookup(const int2* __restrict__ pairs, int64_t q, int32_t blk0,
                                                  int32_t blk1, Table tb, double* __restrict__ lat,
                                                  double* __restrict__ rel, uint8_t* __restrict__ ok) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < q; i += (int64_t)gridDim.x * BLOCK) {
        const int2 p = pairs[i];
        const int32_t sb = p.x >> 6;
        double L = -1.0, R = -1.0;
        // p.x < A: the lanes of the last block past A are padding (no source), and on
        // caller-owned or gathered storage they hold whatever the caller left there
        if (p.x >= 0 && p.x < tb.A && p.y >= 0 && p.y < tb.A && sb >= blk0 && sb < blk1) {
            const size_t o = tidx(sb - blk0, tb.A, p.y, p.x & (WAVE - 1));
            if constexpr (NT) {   // no L2 allocation for a record that is never re-read
                const dvec2 e = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(tb.lr + o));
                L = e.x;
                R = e.y;
            } else {
                const double2 e = tb.lr[o];
                L = e.x;
                R = e.y;
            }
        }
        if constexpr (NT) {
            __builtin_nontemporal_store(L, lat + i);
            __builtin_nontemporal_store(R, rel + i);
        } else {
            lat[i] = L;
            rel[i] = R;
        }
        ok[i] = L > -1.0 ? 1 : 0;   // topology_isRoutable: getLatency > -1
    }
}

// SB64 elements ((block - blk0) * A + t) * 64 + lane; lanes of the last block at
// or past A are padding (no source) and never count
__global__ __launch_bounds__(BLOCK) void k_min_latency(const double2* __restrict__ lr, int64_t elems, int32_t A,
                                                       int32_t blk0, unsigned long long* out) {
    double m = INF;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < elems; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t slot = (i / ((int64_t)A * WAVE) + blk0) * WAVE + (i & (WAVE - 1));
        if (slot >= A) continue;
        const double l = lr[i].x;
        if (l > -1.0 && l < m) m = l;
    }
    for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off));
    if ((threadIdx.x & (WAVE - 1)) == 0 && m < INF)
        atomicMin(out, (unsigned long long)__double_as_longlong(m));  // positive doubles order as integers
}


