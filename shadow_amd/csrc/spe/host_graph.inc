// host_graph.inc -- part of spe.hip (one translation unit).
// Host side: the graph and table objects, device allocation helpers, graph
// creation and upload, the error API.

// ================================================================== host side

struct spe_graph {
    spe::HostGraph hg;
    uint64_t key = 0;              // hash of the graph description (table cache key)
    int32_t device = 0;
    std::vector<double> aux_edge;  // spe_graph_set_edge_aux values per edge (re-uploaded by clones)
    DevGraph dev{};
    HeavyPlan hp{};
    const uint8_t* d_heavy = nullptr;
    DevGraph devx{};               // degree-3 contracted relaxation graph (hg.cx.active), batch engine
    HeavyPlan hpx{};
    std::vector<void*> allocs;
};

struct spe_table {
    spe_graph* g = nullptr;
    uint64_t key = 0;              // on-disk cache key (spe_table_key)
    int32_t A = 0;
    int32_t blk0 = 0, blk1 = 0;
    int32_t row_base = 0;          // the block tb's pointers start at (blk0; spe_table_build_blocks_into moves it)
    int32_t groups = 8;            // 64-source blocks per batch
    int32_t lanes = 16;            // sources per lane group (L)
    int32_t engine = SPE_ENGINE_BATCH;   // resolved engine
    int32_t relax_kernel = SPE_RELAX_REGISTER;   // resolved SPE_RELAX_* (batch engine)
    int32_t infl = 8;              // neighbour rows per round trip (register: in flight per wave; ring: LDS slots)
    bool trace = false;            // per-launch times to stderr while profiling (spe_table_opts.trace)
    unsigned long long* d_lds_dbg = nullptr;       // diagnostic (SPE_LDS_DEBUG): LDS engine phase clocks
#ifdef SPE_DIAGNOSTICS
    bool lds_debug = getenv("SPE_LDS_DEBUG") != nullptr;   // diagnostic builds only
#else
    static constexpr bool lds_debug = false;
#endif
    int32_t occ = 0;               // waves/SIMD the relaxation kernel is held to (0 = compiler's choice)
    // the batch engine's relaxation graph: the core, or its degree-3 contraction (cx)
    bool cx = false;
    const DevGraph* bG = nullptr;
    const HeavyPlan* bhp = nullptr;
    int32_t bn = 0;                // relaxation vertices (state rows per lane group)
    int32_t bm = 0;                // relaxation in-entries
    RowMode md{};
    bool ext = false;
    bool built = false;              // every owned block holds its rows
    std::vector<uint8_t> blk_built;  // per owned block (spe_table_build_blocks builds ranges)
    spe::MultiDev* multi = nullptr;  // a multi-device table: everything below is unused
    Table tb{};
    int32_t* d_slot_vertex = nullptr;
    SlotInfo* d_slots = nullptr;   // row passes (both engines): per-target constants
    bool pend_targets = false;     // some attached target is a pruned pendant (SlotInfo.kt >= 0)
    LdsScratch lsc{};              // LDS engine: per-workgroup parent-entry scratch
    int32_t lds_grid = 0;          // LDS engine: workgroups per launch (scratch is sized for it)
    int32_t* d_rank = nullptr;     // owner replay: position of each slot in the source-run order
    int32_t* d_vertex_slot = nullptr;
    std::vector<int32_t> attached;
    // workspace
    State st{};
    inflag_t* inflag[2] = {nullptr, nullptr};
    uint8_t* mark[2] = {nullptr, nullptr};
    uint8_t* hmark[2] = {nullptr, nullptr};
    Partial pp{};
    int32_t* counts = nullptr;   // per round: 1 if any vertex changed
    unsigned long long* rpend[2] = {nullptr, nullptr};   // route pass: [group][vertex][2] pending lane bits
    int32_t* rcounts = nullptr;  // route pass, per round: 1 if some lane is still pending
    int32_t last_route_rounds = 0;
    unsigned long long* fbound[3] = {nullptr, nullptr, nullptr};   // settle bounds (Flags.fb_*), rotated per round
    unsigned long long* rstats = nullptr;                           // SPE_RELAX_STATS builds only
    unsigned long long* tight = nullptr;   // online margin proof (Flags.tight): [group][vertex][2] lane bits
    bool mg_track = false;                 // this batch's relaxation tracks the margins (build_shared)
    double mg_invw = 0.0, mg_omax = 0.0, mg_hmax = 0.0;
    int32_t max_iters = 0;
    int32_t last_rounds = 0;      // rounds the previous batch needed (sizes the next chunk)
    int32_t* d_srcv = nullptr;     // batch sources, original ids (-1 = padding)
    int32_t* d_srcc = nullptr;     // relaxation ids (-2 = pruned pendant source, -1 = padding)
    int32_t* h_srcv = nullptr;     // pinned staging for both
    int32_t* h_counts = nullptr;
    unsigned long long* d_min = nullptr;
    hipStream_t stream = nullptr;
    // batch engine: the rows of batch i (rows_stream) overlap batch i+1's
    // relaxation (stream) on the other state / source buffer
    bool overlap = false;
    State st_buf[2]{};
    int32_t* srcv_buf[2] = {nullptr, nullptr};
    int32_t* srcc_buf[2] = {nullptr, nullptr};
    hipStream_t rows_stream = nullptr;
    hipEvent_t ev_relaxed = nullptr;
    hipEvent_t ev_rows[2] = {nullptr, nullptr};
    bool rows_pending[2] = {false, false};
    spe_build_stats stats{};
    std::vector<void*> allocs;
    // profiling: one event pair per launch, resolved after each batch's sync
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;
    struct Rec {
        int kind;
        hipEvent_t a, b;
    };
    std::vector<Rec> pending;
    size_t ev_next = 0;
    spe_kernel_profile kp{};
    std::vector<int32_t> h_hist;
    // FW engine: the closure (D, R, N over the relaxation graph, ld x ld), computed
    // by the first build and kept for the table's lifetime
    Fw3 fw{};
    int64_t fw_ld = 0;
    bool fw_done = false;
    // experimental Delta-stepping schedule of the batch engine (SPE_DELTA=<ms> at creation)
    double delta = 0.0;
    DeltaState ds{};
    // shared anchor trees (batch engine, DESIGN §4.1): relaxation lanes = the batch's
    // roots; rows per source through rlane
    bool share = false;
    bool share_off = false;        // this build runs one lane per source (fallback, source trees)
    int32_t* rsrc_buf[2] = {nullptr, nullptr};    // per source slot of the batch: original id (-1 pad)
    int2* rli_buf[2] = {nullptr, nullptr};        // per source slot: {root's state lane, first hop / -1}
    double2* rwa_buf[2] = {nullptr, nullptr};     // per source slot: {pendant latency, f_s (1 - p)}
    int2* rng_buf[2] = {nullptr, nullptr};        // per tile of RT_B source blocks: root lane span
    unsigned char* h_rows = nullptr;   // pinned staging for the three (owned blocks x 64 x 28 B)
    uint8_t* d_unsafe = nullptr;   // per root lane: k_share_check's flag
    uint8_t* h_unsafe = nullptr;
    // contracted shared tables: derived sources (k_rows_derived)
    DLeg* d_der = nullptr;         // the batch's legs (every source slot: its leg range in rli_buf)
    DLeg* h_der = nullptr;         // pinned staging
    size_t leg_cap = 0;            // legs the buffers hold (owned slots x the most legs of a source)
    uint8_t* d_sunsafe = nullptr;  // per source slot of the batch: a derived row's margin failed
    double* d_dx = nullptr;        // [lane group][removed vertex][L]: expanded entries (k_expand_removed)
    Route* d_rtx = nullptr;
    double* d_xd = nullptr;        // SPE_ROWS_LM: [root lane][target slot] staged values (k_stage_lanes)
    Route* d_xrt = nullptr;        //   ... and routes
    const int32_t* d_rorig = nullptr;   // [removed] original id
    int32_t nr = 0;
    uint8_t* h_sunsafe = nullptr;
    bool derive = false;           // contracted sources take their neighbours' roots (no lane)
    // spe_table_opts.exact_delivery (DESIGN §4.1): flagged entries of the shared rows are re-folded
    bool delivery = false;         // the shared build flags and re-folds
    int32_t dl_fallback = 0;       // 1: every edge latency on the ns grid, created as exact_sources = 1
    int32_t dl_cap = 0;            // worklist records per 64-source block
    uint32_t* d_dlcnt = nullptr;   // per block of the batch: flagged entries, then (k_refold_delivery) changed ones
    int4* d_dlwork = nullptr;      // [owned blocks][dl_cap] records (Deliv)
    uint32_t* h_dl = nullptr;      // pinned copy of both
    hipEvent_t ev_dl[2] = {nullptr, nullptr};   // around the re-fold pass (delivery_seconds)
    // spe_lookup_batch_host / spe_table_get: device + pinned staging, grown on demand,
    // one caller at a time (the topology shim queries from several worker threads)
    struct HostLookup {
        std::mutex mu;
        int32_t device = -1;
        hipStream_t stream = nullptr;       // (= sstream[0])
        int64_t cap = 0;                    // queries per staging slot
        // two staging slots (streams, device and pinned buffers): chunk k + 1's transfers and
        // lookups run while chunk k's answers are copied out
        hipStream_t sstream[2] = {nullptr, nullptr};
        int2* d_pairs[2] = {nullptr, nullptr};
        double* d_lat[2] = {nullptr, nullptr};
        double* d_rel[2] = {nullptr, nullptr};
        uint8_t* d_ok[2] = {nullptr, nullptr};
        int2* h_pairs[2] = {nullptr, nullptr};
        double* h_lat[2] = {nullptr, nullptr};
        double* h_rel[2] = {nullptr, nullptr};
        uint8_t* h_ok[2] = {nullptr, nullptr};
        unsigned char* h_entry = nullptr;   // spe_table_get: 16 + 4 + 2 B read back with one sync
        double* d_row = nullptr;            // spe_table_get_row_latrel: one row's lat | rel (2 A)
        double* h_row = nullptr;
    };
    HostLookup* hlk = new HostLookup();
    // Single entries read by host loads (table_host_reads): -1 not decided yet, 0 no, 1 yes
    mutable std::atomic<int> host_rd{-1};
    // Pre-fault of the host mapping (host_prefault_start): 0 not started, 1 running, 2 done,
    // -1 off; the workers, their stop flag and the seconds they took
    mutable std::atomic<int> pf_state{0};
    mutable std::atomic<bool> pf_stop{false};
    mutable std::atomic<int> pf_left{0};
    mutable std::atomic<int64_t> pf_ns{0}, pf_t0{0};
    mutable std::vector<std::thread> pf_threads;
};

namespace {

template <typename T>
int dev_alloc(std::vector<void*>& allocs, T** p, size_t count) {
    void* q = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(&q, count * sizeof(T));
    if (e != hipSuccess)
        return fail(SPE_ENOMEM, "hipMalloc(" + std::to_string(count * sizeof(T)) + " B): " + hipGetErrorString(e));
    allocs.push_back(q);
    *p = static_cast<T*>(q);
    return SPE_OK;
}

template <typename T>
int dev_upload(std::vector<void*>& allocs, const std::vector<T>& h, const T** out) {
    T* p = nullptr;
    int r = dev_alloc(allocs, &p, h.size());
    if (r) return r;
    if (!h.empty()) HIP_TRY(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = p;
    return SPE_OK;
}

int check_device(int32_t device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(SPE_ENODEV, "no HIP device visible");
    if (device < 0 || device >= cnt) return fail(SPE_EINVAL, "device index out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SPE_ENODEV, std::string("libspe is built for gfx950, device is ") + prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    return SPE_OK;
}

// The relaxation shapes instantiated in relax_to_convergence (keep in sync).
#define RELAX_DEFAULT_128 SPE_RELAX_LDS_RING
#ifndef RELAX_RING_NS
#define RELAX_RING_NS 5   // 5 LDS slots per wave at 7 waves / SIMD (MEASUREMENTS.md, round 3)
#endif
#ifndef SPE_RING_OCC
#define SPE_RING_OCC 7    // waves / SIMD of the default ring shape (A/B round 4, 6 / 5 / 4: within the ±3 % box noise of 7)
#endif
bool relax_shape_supported(int32_t lanes, int32_t kernel, int32_t infl, int32_t occ, bool delta) {
    if (delta) return true;   // fixed shapes
    if (lanes == 64) return infl == 8 && occ <= 1;
    if (kernel == SPE_RELAX_LDS_RING)
        return (infl == 4 && occ == 8) || (infl == 5 && occ == SPE_RING_OCC) || (infl == 6 && occ == 6);
    return (infl == 4 && occ <= 1) || (infl == 2 && (occ <= 1 || occ == 6));
}

int grid_for(int64_t work_items, int64_t per_block, int cap = 8192) {
    int64_t b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

}  // namespace

static int graph_upload(spe_graph* g);

int spe::set_error(int code, const std::string& msg) { return fail(code, msg); }

extern "C" {

const char* spe_last_error(void) { return g_err.c_str(); }

int spe_device_count(int32_t* out) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    if (out) *out = c;
    return SPE_OK;
}

int spe_graph_create(const spe_graph_desc* desc, int32_t device, spe_graph** out) {
    if (!out) return fail(SPE_EINVAL, "out is NULL");
    if (desc && desc->struct_size != sizeof(spe_graph_desc)) return fail(SPE_EINVAL, ABI_MSG("spe_graph_desc"));
    *out = nullptr;
    auto* g = new spe_graph();
    std::string err;
    int r = spe::prepare_graph(desc, &g->hg, &err);
    if (r) {
        delete g;
        return fail(r, err);
    }
    r = check_device(device);
    if (r) {
        delete g;
        return r;
    }
    g->device = device;
    {   // everything in the description that can change a row
        Fnv f;
        f.val(desc->n_vertices);
        f.val(desc->n_edges);
        const size_t m = (size_t)desc->n_edges;
        f.add(desc->edge_source, m * sizeof(int32_t));
        f.add(desc->edge_target, m * sizeof(int32_t));
        f.add(desc->edge_latency, m * sizeof(double));
        f.add(desc->edge_packetloss, m * sizeof(double));
        const int32_t has_v = desc->vertex_packetloss != nullptr;
        f.val(has_v);
        if (has_v) f.add(desc->vertex_packetloss, (size_t)desc->n_vertices * sizeof(double));
        f.val(desc->directed);
        f.val(desc->prefer_direct);
        g->key = f.h;
    }
    spe::prune_pendants(&g->hg, desc->keep_pendants == 0);
    spe::contract_degree3(&g->hg);
    spe::share_prep(&g->hg);
    r = graph_upload(g);
    if (r) {
        spe_graph_free(g);
        return r;
    }
    *out = g;
    return SPE_OK;
}

}  // extern "C"

// Device copy of a prepared host graph (spe_graph_create, and the other devices
// of a multi-device table).  On failure the caller frees g.
static int graph_upload(spe_graph* g) {
    int r = SPE_OK;
    const spe::HostGraph& h = g->hg;
    DevGraph& d = g->dev;
    d.n = h.nc;
    d.n_full = h.n;
    d.nrel = (int32_t)h.icol.size();
#ifdef SPE_DIAGNOSTICS   // experiments only: SPE_ABLATE bit 0 skips route records (inexact rows)
    d.ablate = getenv("SPE_ABLATE") ? atoi(getenv("SPE_ABLATE")) : 0;
#else
    d.ablate = 0;
#endif
#define UPBASE d
#define UP(field, src)                                   \
    do {                                                 \
        r = dev_upload(g->allocs, src, &UPBASE.field);   \
        if (r) return r;                                 \
    } while (0)
    UP(iptr, h.iptr);
    UP(icol, h.icol);
    {
        std::vector<int32_t> irow(h.icol.size());
        for (int32_t v = 0; v < h.nc; ++v)
            for (int32_t k = h.iptr[v]; k < h.iptr[v + 1]; ++k) irow[k] = v;
        r = dev_upload(g->allocs, irow, &d.irow);
        if (r) return r;
        d.ipair = nullptr;
        if (h.nc <= 65535) {
            std::vector<uint32_t> ip(h.icol.size());
            for (size_t k = 0; k < ip.size(); ++k) ip[k] = ((uint32_t)irow[k] << 16) | (uint32_t)h.icol[k];
            r = dev_upload(g->allocs, ip, &d.ipair);
            if (r) return r;
        }
    }
    UP(iw, h.iw);
    UP(ia, h.ia);
    UP(iwrep, h.iwrep);
    UP(orev, h.orev);
    if (h.directed) {
        UP(optr, h.optr);
        UP(ocol, h.ocol);
        UP(owrep, h.owrep);
        UP(oarep, h.oarep);
        UP(ow, h.ow);
        d.undirected = 0;
    } else {
        d.optr = d.iptr;
        d.ocol = d.icol;
        d.owrep = d.iwrep;
        d.oarep = d.ia;
        d.ow = d.iw;
        d.undirected = 1;
    }
    UP(vfac, h.vfac);
    UP(loop_w, h.loop_w);
    UP(loop_a, h.loop_a);
    UP(self_w2, h.self_w2);
    UP(self_a2, h.self_a2);
    UP(self_other, h.self_other);
    UP(core_id, h.core_id);
    UP(corev, h.corev);
    UP(anchor_core, h.anchor_core);
    UP(fiptr, h.fiptr);
    UP(fiw, h.fiw);
    UP(fia, h.fia);
    UP(fiwrep, h.fiwrep);
    if (h.directed) {
        d.dptr = d.optr;
        d.dcol = d.ocol;
        d.dwrep = d.owrep;
        d.darep = d.oarep;
    } else if (!h.pruned) {
        d.dptr = d.iptr;
        d.dcol = d.icol;
        d.dwrep = d.iwrep;
        d.darep = d.ia;
    } else {
        d.dptr = d.fiptr;
        UP(dcol, h.ficol);
        d.dwrep = d.fiwrep;
        d.darep = d.fia;
    }
    {   // heavy-vertex segment plan (in-degree > 64), over the relaxation graph
        std::vector<uint8_t> heavy(h.nc, 0);
        std::vector<int32_t> seg_vertex, seg_begin, heavy_vertex, heavy_seg0;
        for (int32_t v = 0; v < h.nc; ++v) {
            const int32_t k0 = h.iptr[v], k1 = h.iptr[v + 1];
            if (k1 - k0 <= WAVE) continue;
            heavy[v] = 1;
            heavy_vertex.push_back(v);
            heavy_seg0.push_back((int32_t)seg_vertex.size());
            for (int32_t k = k0; k < k1; k += WAVE) {
                seg_vertex.push_back(v);
                seg_begin.push_back(k);
            }
        }
        heavy_seg0.push_back((int32_t)seg_vertex.size());
        g->hp.nseg = (int32_t)seg_vertex.size();
        g->hp.nheavy = (int32_t)heavy_vertex.size();
#undef UPBASE
#define UPBASE g->hp
        UP(seg_vertex, seg_vertex);
        UP(seg_begin, seg_begin);
        UP(heavy_vertex, heavy_vertex);
        UP(heavy_seg0, heavy_seg0);
#undef UPBASE
        r = dev_upload(g->allocs, heavy, &g->d_heavy);
        if (r) return r;
        d.heavy = g->d_heavy;
        const std::vector<int32_t>& oc = h.directed ? h.ocol : h.icol;
        std::vector<uint8_t> oheavy(oc.size());
        for (size_t k = 0; k < oc.size(); ++k) oheavy[k] = heavy[oc[k]];
        r = dev_upload(g->allocs, oheavy, &d.oheavy);
        if (r) return r;
        std::vector<int4> pack(std::max<size_t>(1, h.icol.size()));
        for (size_t k = 0; k < h.icol.size(); ++k) {
            uint64_t wb;
            std::memcpy(&wb, &h.iw[k], sizeof wb);
            const int32_t rev = h.directed ? 0 : (h.orev[k] | (heavy[h.icol[k]] ? (int32_t)0x80000000 : 0));
            pack[k] = make_int4(h.icol[k], rev, (int32_t)(uint32_t)wb, (int32_t)(uint32_t)(wb >> 32));
        }
        r = dev_upload(g->allocs, pack, &d.ipack);
        if (r) return r;
    }
#undef UP
    if (h.cx.active) {   // the batch engine's contracted relaxation graph (shares the rest of dev)
        const spe::HostGraph::Contracted& cx = h.cx;
        DevGraph& x = g->devx;
        x = d;
        x.n = cx.nk;
        x.nrel = (int32_t)cx.col.size();
        x.ipair = nullptr;
        x.iaux = x.fiaux = nullptr;
#define UPX(field, src)                                  \
    do {                                                 \
        r = dev_upload(g->allocs, src, &x.field);        \
        if (r) return r;                                 \
    } while (0)
        UPX(iptr, cx.ptr);
        UPX(icol, cx.col);
        UPX(iw, cx.w1);
        UPX(ia, cx.a1);
        UPX(orev, cx.rev);
        UPX(xw2, cx.w2);
        UPX(xa2, cx.a2);
        UPX(xkey, cx.key);
        UPX(xvia, cx.via);
        UPX(rnb, cx.rnb);
        UPX(rw, cx.rw);
        UPX(ra, cx.ra);
        x.iwrep = x.iw;   // (contraction needs no multigraph representatives)
        x.optr = x.iptr;
        x.ocol = x.icol;
        x.owrep = x.iw;
        x.oarep = x.ia;
        x.ow = x.iw;
        {
            std::vector<int32_t> irow(cx.col.size()), cid(h.n, -1), anc(h.n, -1), rm(h.n, -1);
            for (int32_t v = 0; v < cx.nk; ++v)
                for (int32_t k = cx.ptr[v]; k < cx.ptr[v + 1]; ++k) irow[k] = v;
            std::vector<int32_t> corev(cx.nk);
            for (int32_t k = 0; k < cx.nk; ++k) corev[k] = h.corev[cx.kcore[k]];
            for (int32_t v = 0; v < h.n; ++v) {
                const int32_t c = h.core_id[v];
                if (c >= 0) {
                    cid[v] = cx.kid[c];
                    rm[v] = cx.rid[c];
                } else if (h.anchor_core[v] >= 0) {
                    anc[v] = cx.kid[h.anchor_core[v]];   // (no removed vertex anchors a pendant)
                }
            }
            UPX(irow, irow);
            UPX(corev, corev);
            UPX(core_id, cid);
            UPX(anchor_core, anc);
            UPX(xrm, rm);
        }
#undef UPX
        std::vector<uint8_t> heavy(cx.nk, 0);
        std::vector<int32_t> seg_vertex, seg_begin, heavy_vertex, heavy_seg0;
        for (int32_t v = 0; v < cx.nk; ++v) {
            const int32_t k0 = cx.ptr[v], k1 = cx.ptr[v + 1];
            if (k1 - k0 <= WAVE) continue;
            heavy[v] = 1;
            heavy_vertex.push_back(v);
            heavy_seg0.push_back((int32_t)seg_vertex.size());
            for (int32_t k = k0; k < k1; k += WAVE) {
                seg_vertex.push_back(v);
                seg_begin.push_back(k);
            }
        }
        heavy_seg0.push_back((int32_t)seg_vertex.size());
        g->hpx.nseg = (int32_t)seg_vertex.size();
        g->hpx.nheavy = (int32_t)heavy_vertex.size();
        if ((r = dev_upload(g->allocs, seg_vertex, &g->hpx.seg_vertex))) return r;
        if ((r = dev_upload(g->allocs, seg_begin, &g->hpx.seg_begin))) return r;
        if ((r = dev_upload(g->allocs, heavy_vertex, &g->hpx.heavy_vertex))) return r;
        if ((r = dev_upload(g->allocs, heavy_seg0, &g->hpx.heavy_seg0))) return r;
        if ((r = dev_upload(g->allocs, heavy, &x.heavy))) return r;
        std::vector<uint8_t> oheavy(cx.col.size());
        for (size_t k = 0; k < cx.col.size(); ++k) oheavy[k] = heavy[cx.col[k]];
        if ((r = dev_upload(g->allocs, oheavy, &x.oheavy))) return r;
        // bit 31: the target of the reverse entry is heavy; bit 30: a shortcut entry
        std::vector<int4> pack(std::max<size_t>(1, cx.col.size()));
        for (size_t k = 0; k < cx.col.size(); ++k) {
            uint64_t wb;
            std::memcpy(&wb, &cx.w1[k], sizeof wb);
            const int32_t rev = cx.rev[k] | (cx.via[k] >= 0 ? 0x40000000 : 0) | (heavy[cx.col[k]] ? (int32_t)0x80000000 : 0);
            pack[k] = make_int4(cx.col[k], rev, (int32_t)(uint32_t)wb, (int32_t)(uint32_t)(wb >> 32));
        }
        if ((r = dev_upload(g->allocs, pack, &x.ipack))) return r;
    }
    if (!g->aux_edge.empty()) {   // the auxiliary attribute, if set (spe_graph_set_edge_aux)
        std::vector<double> ia(h.ieid.size()), fa(h.fieid.size());
        for (size_t k = 0; k < ia.size(); ++k) ia[k] = g->aux_edge[h.ieid[k]];
        for (size_t k = 0; k < fa.size(); ++k) fa[k] = g->aux_edge[h.fieid[k]];
        if (ia.empty()) ia.push_back(0.0);
        if (fa.empty()) fa.push_back(0.0);
        if ((r = dev_upload(g->allocs, ia, &g->dev.iaux))) return r;
        if ((r = dev_upload(g->allocs, fa, &g->dev.fiaux))) return r;
    }
    return SPE_OK;
}

int spe::graph_clone(const spe_graph* g, int32_t device, spe_graph** out) {
    *out = nullptr;
    int r = check_device(device);
    if (r) return r;
    auto* c = new spe_graph();
    c->hg = g->hg;
    c->key = g->key;
    c->device = device;
    c->aux_edge = g->aux_edge;
    r = graph_upload(c);
    if (r) {
        spe_graph_free(c);
        return r;
    }
    *out = c;
    return SPE_OK;
}

