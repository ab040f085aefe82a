// host_api.inc -- part of spe.hip (one translation unit).
// Host side: reads (entries, downloads, lookups), the table check, the FW
// comparison closure, source trees and the on-disk table cache.

// ---- single entries by host loads.  On a large-BAR host the device's memory is mapped
// into this process (measured on the MI355X boxes, tools/probe_single_call.hip: a 16-B
// host load of a record in hipMalloc memory takes ~2.6 us and returns the device's
// values, against ~11 us for hipMemcpyAsync + synchronisation), so a per-packet read
// (shd-worker.c:235-247 -> spe_table_get_latrel) needs no DMA, no stream and no lock.
// Decided once per table: the record span must be mapped readable in /proc/self/maps
// and two records read both ways must agree bit for bit; SPE_HOST_READS=0 turns it
// off.  Builds end with a system-scope release (k_release_system), so the host sees
// every record the kernels wrote.
typedef double host_v2d __attribute__((vector_size(16)));

// one 16-B load: both halves of the record in one PCIe read
static inline void host_load_latrel(const double2* p, double* latency, double* reliability) {
    const host_v2d h = *reinterpret_cast<const volatile host_v2d*>(p);
    *latency = h[0];
    *reliability = h[1];
}

static bool mapped_readable(const void* p, size_t bytes) {
    FILE* f = fopen("/proc/self/maps", "r");
    if (!f) return false;
    uintptr_t want = (uintptr_t)p;
    const uintptr_t end = want + bytes;
    char line[512];
    while (want < end && fgets(line, sizeof line, f)) {
        unsigned long long a = 0, b = 0;
        char perm[8] = {0};
        if (sscanf(line, "%llx-%llx %7s", &a, &b, perm) != 3) continue;
        if (a <= want && want < b) {
            if (perm[0] != 'r') break;
            want = (uintptr_t)b;   // the span may continue in the next mapping
        }
    }
    fclose(f);
    return want >= end;
}

// The first host load of each page of the mapping takes a page fault in the driver (the
// fault maps a 64-KB window: 16 pages), and the faults of one allocation serialise:
// measured on the boxes (tools/exp_host_reads_mt.py, profiles/r06_prefault*.log), random
// get_latrel calls on the C4 table run at 225k/s on one thread and 360k/s on 16 while the
// mapping fills, 760k/s and 8.4M/s once it is filled.  So the first host read starts a
// background thread that loads one byte of every 64-KB window of the latrel field (the
// per-packet read; next_hop / hops fault on use); spe_table_free stops and joins it.
// More threads only contend for the same lock (C4, all three fields: 14.1 s on one
// thread, 20.0 s on 4, 16.8 s on 16), and slow the foreground reads meanwhile.
static void host_prefault_start(const spe_table* t) {
    int expect = 0;
    const char* e = getenv("SPE_HOST_PREFAULT");
    const int nt = e && *e ? std::min(64, std::max(0, atoi(e))) : 1;
    if (nt == 0) {
        t->pf_state.compare_exchange_strong(expect, -1);
        return;
    }
    if (!t->pf_state.compare_exchange_strong(expect, 1)) return;
    const size_t elems = (size_t)(t->blk1 - t->blk0) * t->A * WAVE;
    struct Span {
        const unsigned char* p;
        size_t bytes;
    };
    const Span spans[1] = {{(const unsigned char*)t->tb.lr, elems * sizeof(double2)}};
    constexpr size_t WIN = 64 << 10;
    const auto t0 = std::chrono::steady_clock::now();
    t->pf_t0.store(std::chrono::duration_cast<std::chrono::nanoseconds>(t0.time_since_epoch()).count());
    t->pf_left.store(nt);
    for (int k = 0; k < nt; ++k) try {
        t->pf_threads.emplace_back([t, k, nt, spans, t0] {
            for (const Span& s : spans) {
                if (!s.p) continue;
                const size_t wins = (s.bytes + WIN - 1) / WIN, w0 = wins * k / nt, w1 = wins * (k + 1) / nt;
                for (size_t w = w0; w < w1 && !t->pf_stop.load(std::memory_order_relaxed); ++w)
                    (void)*reinterpret_cast<const volatile unsigned char*>(s.p + w * WIN);
            }
            if (t->pf_left.fetch_sub(1) == 1) {   // the last one out records the time
                const auto ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0);
                t->pf_ns.store((int64_t)ns.count(), std::memory_order_release);
                t->pf_state.store(t->pf_stop.load() ? 1 : 2, std::memory_order_release);
            }
        });
    } catch (...) {   // no thread: the mapping fills on use, as without the pre-fault
        if (t->pf_left.fetch_sub(nt - k) == nt - k) t->pf_state.store(-1, std::memory_order_release);
        break;
    }
}

static void host_prefault_stop(spe_table* t) {
    t->pf_stop.store(true);
    for (std::thread& th : t->pf_threads)
        if (th.joinable()) th.join();
    t->pf_threads.clear();
}

static bool table_host_reads(const spe_table* t) {
    const int v = t->host_rd.load(std::memory_order_acquire);
    if (v >= 0) return v != 0;
    const char* e = getenv("SPE_HOST_READS");
    int ok = 0;
    if (!(e && *e == '0') && t->tb.lr && !t->multi) {
        int32_t b = -1;   // a built block to verify on
        for (int32_t i = 0; i < t->blk1 - t->blk0 && b < 0; ++i)
            if (t->blk_built[(size_t)i]) b = t->blk0 + i;
        if (b < 0) return false;   // nothing built yet: decide later
        const size_t elems = (size_t)(t->blk1 - t->blk0) * t->A * WAVE;
        if (mapped_readable(t->tb.lr, elems * sizeof(double2)) && mapped_readable(t->tb.next, elems * sizeof(int32_t)) &&
            mapped_readable(t->tb.hops, elems * sizeof(uint16_t))) {
            ok = 1;
            const size_t base = (size_t)(b - t->blk0) * t->A * WAVE;
            for (size_t o : {base, base + (size_t)t->A * WAVE - 1}) {
                double2 d{};
                if (hipMemcpy(&d, t->tb.lr + o, sizeof d, hipMemcpyDeviceToHost) != hipSuccess) {
                    ok = 0;
                    break;
                }
                double hl = 0.0, hr = 0.0;
                host_load_latrel(t->tb.lr + o, &hl, &hr);
                ok &= std::memcmp(&d.x, &hl, 8) == 0 && std::memcmp(&d.y, &hr, 8) == 0;
            }
        }
    }
    int undecided = -1;
    if (t->host_rd.compare_exchange_strong(undecided, ok, std::memory_order_acq_rel) && ok) host_prefault_start(t);
    return ok != 0;
}

extern "C" {

int spe_table_get(const spe_table* t, int32_t s_slot, int32_t t_slot, spe_entry* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) {
        if (!t->built) return fail(SPE_ESTATE, "table not built");
        return spe::multi_get(t->multi, s_slot, t_slot, out);
    }
    if (s_slot < 0 || s_slot >= t->A || t_slot < 0 || t_slot >= t->A) return fail(SPE_EINVAL, "slot out of range");
    const int32_t sb = s_slot / WAVE;
    if (sb < t->blk0 || sb >= t->blk1) return fail(SPE_EINVAL, "source row not owned by this table");
    if (!t->blk_built[(size_t)(sb - t->blk0)]) return fail(SPE_ESTATE, "source row not built");
    const size_t o = ((size_t)(sb - t->blk0) * t->A + t_slot) * WAVE + (s_slot % WAVE);
    if (table_host_reads(t)) {
        host_load_latrel(t->tb.lr + o, &out->latency, &out->reliability);
        out->next_hop = *reinterpret_cast<const volatile int32_t*>(t->tb.next + o);
        out->hops = *reinterpret_cast<const volatile uint16_t*>(t->tb.hops + o);
        return SPE_OK;
    }
    HIP_TRY(hipSetDevice(t->g->device));
    // the three fields read back into pinned memory on one stream, one synchronisation
    spe_table::HostLookup* hl = t->hlk;
    std::lock_guard<std::mutex> lock(hl->mu);
    if (int r = host_lookup_reserve(hl, t->g->device, 0)) return r;
    unsigned char* b = hl->h_entry;
    HIP_TRY(hipMemcpyAsync(b, t->tb.lr + o, sizeof(double2), hipMemcpyDeviceToHost, hl->stream));
    HIP_TRY(hipMemcpyAsync(b + 16, t->tb.next + o, sizeof(int32_t), hipMemcpyDeviceToHost, hl->stream));
    HIP_TRY(hipMemcpyAsync(b + 20, t->tb.hops + o, sizeof(uint16_t), hipMemcpyDeviceToHost, hl->stream));
    HIP_TRY(hipStreamSynchronize(hl->stream));
    double2 e;
    uint16_t h = 0;
    std::memcpy(&e, b, sizeof e);
    std::memcpy(&out->next_hop, b + 16, sizeof(int32_t));
    std::memcpy(&h, b + 20, sizeof h);
    out->latency = e.x;
    out->reliability = e.y;
    out->hops = h;
    return SPE_OK;
}

int spe_table_get_latrel(const spe_table* t, int32_t s_slot, int32_t t_slot, double* latency, double* reliability) {
    if (!t || !latency || !reliability) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) {
        spe_entry e;
        if (int r = spe_table_get(t, s_slot, t_slot, &e)) return r;
        *latency = e.latency;
        *reliability = e.reliability;
        return SPE_OK;
    }
    if (s_slot < 0 || s_slot >= t->A || t_slot < 0 || t_slot >= t->A) return fail(SPE_EINVAL, "slot out of range");
    const int32_t sb = s_slot / WAVE;
    if (sb < t->blk0 || sb >= t->blk1) return fail(SPE_EINVAL, "source row not owned by this table");
    if (!t->blk_built[(size_t)(sb - t->blk0)]) return fail(SPE_ESTATE, "source row not built");
    const size_t o = ((size_t)(sb - t->blk0) * t->A + t_slot) * WAVE + (s_slot % WAVE);
    if (table_host_reads(t)) {
        host_load_latrel(t->tb.lr + o, latency, reliability);
        return SPE_OK;
    }
    HIP_TRY(hipSetDevice(t->g->device));
    spe_table::HostLookup* hl = t->hlk;
    std::lock_guard<std::mutex> lock(hl->mu);
    if (int r = host_lookup_reserve(hl, t->g->device, 0)) return r;
    HIP_TRY(hipMemcpyAsync(hl->h_entry, t->tb.lr + o, sizeof(double2), hipMemcpyDeviceToHost, hl->stream));
    HIP_TRY(hipStreamSynchronize(hl->stream));
    double2 e;
    std::memcpy(&e, hl->h_entry, sizeof e);
    *latency = e.x;
    *reliability = e.y;
    return SPE_OK;
}

// one source row's records out of its SB64 block: lat[t], rel[t] for every target t
__global__ __launch_bounds__(256) void k_row_latrel(int32_t A, const double2* __restrict__ blk, int32_t lane,
                                                    double* __restrict__ out) {
    for (int32_t t = blockIdx.x * 256 + threadIdx.x; t < A; t += gridDim.x * 256) {
        const double2 e = blk[(size_t)t * WAVE + lane];
        out[t] = e.x;
        out[(size_t)A + t] = e.y;
    }
}

int spe_table_get_row_latrel(const spe_table* t, int32_t s_slot, double* latency, double* reliability) {
    if (!t || !latency || !reliability) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return spe_table_download(t, s_slot, s_slot + 1, latency, reliability, nullptr, nullptr);
    if (s_slot < 0 || s_slot >= t->A) return fail(SPE_EINVAL, "slot out of range");
    const int32_t sb = s_slot / WAVE;
    if (sb < t->blk0 || sb >= t->blk1) return fail(SPE_EINVAL, "source row not owned by this table");
    if (!t->blk_built[(size_t)(sb - t->blk0)]) return fail(SPE_ESTATE, "source row not built");
    spe_table::HostLookup* hl = t->hlk;
    std::lock_guard<std::mutex> lock(hl->mu);
    if (int r = host_lookup_reserve(hl, t->g->device, 0)) return r;
    if (!hl->d_row || !hl->h_row) {   // both buffers or neither (a failed allocation leaves none set)
        double* d = nullptr;
        double* h = nullptr;
        hipError_t e = hipMalloc(&d, (size_t)t->A * 2 * sizeof(double));
        if (e == hipSuccess) e = hipHostMalloc((void**)&h, (size_t)t->A * 2 * sizeof(double), hipHostMallocDefault);
        if (e != hipSuccess) {
            if (d) (void)hipFree(d);
            return fail(SPE_EHIP, hipGetErrorString(e));
        }
        if (hl->d_row) (void)hipFree(hl->d_row);
        if (hl->h_row) (void)hipHostFree(hl->h_row);
        hl->d_row = d;
        hl->h_row = h;
    }
    const double2* blk = t->tb.lr + (size_t)(sb - t->blk0) * t->A * WAVE;
    k_row_latrel<<<std::min(1024, (t->A + 255) / 256), 256, 0, hl->stream>>>(t->A, blk, s_slot % WAVE, hl->d_row);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hl->h_row, hl->d_row, (size_t)t->A * 2 * sizeof(double), hipMemcpyDeviceToHost, hl->stream));
    HIP_TRY(hipStreamSynchronize(hl->stream));
    std::memcpy(latency, hl->h_row, (size_t)t->A * sizeof(double));
    std::memcpy(reliability, hl->h_row + t->A, (size_t)t->A * sizeof(double));
    return SPE_OK;
}

// SB64 block -> 64 row-major rows, on the device (a 64 x 64 LDS tile per
// workgroup: coalesced reads of the 64 interleaved sources, coalesced row writes).
__global__ __launch_bounds__(256) void k_sb64_rows(int32_t A, const double2* __restrict__ lr,
                                                   const int32_t* __restrict__ nx, const uint16_t* __restrict__ hp,
                                                   const double* __restrict__ ax, double* __restrict__ olat,
                                                   double* __restrict__ orel, int32_t* __restrict__ onext,
                                                   int32_t* __restrict__ ohops, double* __restrict__ oaux) {
    __shared__ double T0[64][65], T1[64][65];
    __shared__ int32_t I0[64][65], I1[64][65];
    const int32_t j0 = blockIdx.x * 64;
    for (int32_t e = threadIdx.x; e < 64 * 64; e += 256) {   // e = (target jj, lane l), lane fastest
        const int32_t jj = e / 64, l = e % 64, j = j0 + jj;
        if (j >= A) continue;
        const size_t o = (size_t)j * WAVE + l;
        if (olat || orel) {
            const double2 v = lr[o];
            T0[l][jj] = v.x;
            T1[l][jj] = v.y;
        }
        if (oaux) T0[l][jj] = ax[o];
        if (onext) I0[l][jj] = nx[o];
        if (ohops) I1[l][jj] = hp[o];
    }
    __syncthreads();
    for (int32_t e = threadIdx.x; e < 64 * 64; e += 256) {   // e = (lane l, target jj), target fastest
        const int32_t l = e / 64, jj = e % 64, j = j0 + jj;
        if (j >= A) continue;
        const size_t o = (size_t)l * A + j;
        if (olat) olat[o] = T0[l][jj];
        if (orel) orel[o] = T1[l][jj];
        if (oaux) oaux[o] = T0[l][jj];
        if (onext) onext[o] = I0[l][jj];
        if (ohops) ohops[o] = I1[l][jj];
    }
}

// Owned rows [row_begin, row_end) to host, row-major: each 64-source block is
// transposed on the device, then copied as one contiguous span per field.
// (aux is requested alone: it shares the first staging tile with latency.)
static int download_rows(const spe_table* t, int32_t row_begin, int32_t row_end, double* latency,
                         double* reliability, int32_t* next_hop, int32_t* hops, double* aux) {
    if (!t) return fail(SPE_EINVAL, "NULL table");
    if (row_begin < t->blk0 * WAVE || row_end > std::min(t->A, t->blk1 * WAVE) || row_begin > row_end)
        return fail(SPE_EINVAL, "row range not owned by this table");
    for (int32_t b = row_begin / WAVE; b < (row_end + WAVE - 1) / WAVE; ++b)
        if (!t->blk_built[(size_t)(b - t->blk0)]) return fail(SPE_ESTATE, "rows not built");
    if (row_begin == row_end) return SPE_OK;
    HIP_TRY(hipSetDevice(t->g->device));
    const int32_t A = t->A;
    const size_t blk_elems = (size_t)A * WAVE;
    const int32_t b0 = row_begin / WAVE, b1 = (row_end + WAVE - 1) / WAVE;
    // Many blocks (a host mirror): two slots -- block k + 1 is transposed and copied down
    // into pinned staging on its own stream while block k's rows are copied out on
    // several threads (pageable device-to-host copies ran at ~7 GB/s).
    const bool piped = b1 - b0 >= 4;
    const int ns = piped ? 2 : 1;
    std::vector<void*> tmp, pin, reg;
    // Many blocks: the caller's arrays registered with the runtime (hipHostRegister, ~2 ms
    // per GB) take the transposed rows by DMA straight away -- no staging copy on the host
    // (53 GB/s either way on an idle host, tools/probe_single_call.hip; the staging copy
    // is what a loaded host runs out of).  Arrays the runtime refuses go through staging.
    bool direct = false;
    if (piped && !getenv("SPE_DOWNLOAD_STAGED")) {
        const size_t rows = (size_t)(row_end - row_begin) * A;
        direct = true;
        for (auto f : {std::make_pair((void*)latency, (size_t)8), std::make_pair((void*)reliability, (size_t)8),
                       std::make_pair((void*)aux, (size_t)8), std::make_pair((void*)next_hop, (size_t)4),
                       std::make_pair((void*)hops, (size_t)4)}) {
            if (!f.first || !direct) continue;
            const hipError_t e = hipHostRegister(f.first, rows * f.second, hipHostRegisterDefault);
            if (e == hipSuccess) reg.push_back(f.first);
            else if (e != hipErrorHostMemoryAlreadyRegistered) direct = false;
        }
        (void)hipGetLastError();
        if (!direct) {
            for (void* p : reg) (void)hipHostUnregister(p);
            reg.clear();
        }
    }
    double *dl[2] = {}, *dr[2] = {}, *da[2] = {};
    int32_t *dn[2] = {}, *dh[2] = {};
    double *pl[2] = {}, *pr[2] = {}, *pa[2] = {};
    int32_t *pn[2] = {}, *ph[2] = {};
    hipStream_t st[2] = {t->stream, nullptr};
    int r = SPE_OK;
    for (int k = 0; k < ns && !r; ++k) {
        if (latency && !r) r = dev_alloc(tmp, &dl[k], blk_elems);
        if (reliability && !r) r = dev_alloc(tmp, &dr[k], blk_elems);
        if (aux && !r) r = dev_alloc(tmp, &da[k], blk_elems);
        if (next_hop && !r) r = dev_alloc(tmp, &dn[k], blk_elems);
        if (hops && !r) r = dev_alloc(tmp, &dh[k], blk_elems);
        if (!piped) break;
        if (k == 1 && !r && hipStreamCreateWithFlags(&st[1], hipStreamNonBlocking) != hipSuccess)
            r = fail(SPE_EHIP, "hipStreamCreate (download)");
        if (direct) continue;
        auto hmal = [&](auto** p, size_t bytes) {
            void* q = nullptr;
            if (!r && hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) r = fail(SPE_ENOMEM, "hipHostMalloc (download staging)");
            if (q) pin.push_back(q);
            *p = (std::remove_reference_t<decltype(**p)>*)q;
        };
        if (latency) hmal(&pl[k], blk_elems * 8);
        if (reliability) hmal(&pr[k], blk_elems * 8);
        if (aux) hmal(&pa[k], blk_elems * 8);
        if (next_hop) hmal(&pn[k], blk_elems * 4);
        if (hops) hmal(&ph[k], blk_elems * 4);
    }
    // the rows of block b inside [row_begin, row_end): (offset in the block's row-major rows,
    // offset in the caller's arrays, element count)
    auto span = [&](int32_t b, size_t* src, size_t* dst, size_t* cnt) {
        const int32_t r0 = std::max(row_begin, b * WAVE), r1 = std::min(row_end, (b + 1) * WAVE);
        *src = (size_t)(r0 - b * WAVE) * A;
        *dst = (size_t)(r0 - row_begin) * A;
        *cnt = (size_t)(r1 - r0) * A;
    };
    auto issue = [&](int32_t b, int k) -> int {
        const size_t off = (size_t)(b - t->blk0) * blk_elems;
        k_sb64_rows<<<(A + 63) / 64, 256, 0, st[k]>>>(A, t->tb.lr + off, t->tb.next + off, t->tb.hops + off,
                                                      aux ? t->tb.aux + off : nullptr, dl[k], dr[k], dn[k], dh[k], da[k]);
        if (hipGetLastError() != hipSuccess) return fail(SPE_EHIP, "k_sb64_rows launch");
        size_t src, dst, cnt;
        span(b, &src, &dst, &cnt);
        auto cp = [&](void* h, void* p, const void* d, size_t esz) -> int {
            if (!h) return SPE_OK;
            void* to = (piped && !direct) ? (char*)p + src * esz : (char*)h + dst * esz;
            if (hipMemcpyAsync(to, (const char*)d + src * esz, cnt * esz, hipMemcpyDeviceToHost, st[k]) != hipSuccess)
                return fail(SPE_EHIP, "hipMemcpyAsync (download)");
            return SPE_OK;
        };
        int q = cp(latency, pl[k], dl[k], 8);
        if (!q) q = cp(reliability, pr[k], dr[k], 8);
        if (!q) q = cp(aux, pa[k], da[k], 8);
        if (!q) q = cp(next_hop, pn[k], dn[k], 4);
        if (!q) q = cp(hops, ph[k], dh[k], 4);
        return q;
    };
    auto finish = [&](int32_t b, int k) -> int {
        if (hipStreamSynchronize(st[k]) != hipSuccess) return fail(SPE_EHIP, "download sync");
        if (!piped || direct) return SPE_OK;
        size_t src, dst, cnt;
        span(b, &src, &dst, &cnt);
        if (latency) pcopy(latency + dst, pl[k] + src, cnt * 8);
        if (reliability) pcopy(reliability + dst, pr[k] + src, cnt * 8);
        if (aux) pcopy(aux + dst, pa[k] + src, cnt * 8);
        if (next_hop) pcopy(next_hop + dst, pn[k] + src, cnt * 4);
        if (hops) pcopy(hops + dst, ph[k] + src, cnt * 4);
        return SPE_OK;
    };
    for (int32_t b = b0; !r && b < b1; ++b) {
        const int k = piped ? (b - b0) & 1 : 0;
        if (piped && b - b0 >= 2) r = finish(b - 2, k);   // the slot's previous block is out first
        if (!r) r = issue(b, k);
        if (!r && !piped) r = finish(b, 0);
    }
    if (piped)
        for (int32_t b = std::max(b0, b1 - 2); !r && b < b1; ++b) r = finish(b, (b - b0) & 1);
    for (int k = 0; k < 2; ++k)
        if (st[k]) (void)hipStreamSynchronize(st[k]);
    if (st[1]) (void)hipStreamDestroy(st[1]);
    for (void* p : tmp) (void)hipFree(p);
    for (void* p : pin) (void)hipHostFree(p);
    for (void* p : reg) (void)hipHostUnregister(p);
    return r;
}

int spe_table_download(const spe_table* t, int32_t row_begin, int32_t row_end, double* latency,
                       double* reliability, int32_t* next_hop, int32_t* hops) {
    if (t && t->multi) {
        if (!t->built) return fail(SPE_ESTATE, "table not built");
        return spe::multi_download(t->multi, row_begin, row_end, latency, reliability, next_hop, hops);
    }
    return download_rows(t, row_begin, row_end, latency, reliability, next_hop, hops, nullptr);
}

int spe_table_download_aux(const spe_table* t, int32_t row_begin, int32_t row_end, double* aux) {
    if (!t || !aux) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return fail(SPE_EUNSUPPORTED, "multi-device tables have no aux field");
    if (!t->tb.aux) return fail(SPE_ESTATE, "table was created without want_aux");
    return download_rows(t, row_begin, row_end, nullptr, nullptr, nullptr, nullptr, aux);
}

int spe_lookup_batch(const spe_table* t, const int32_t* d_pairs, int64_t q, double* d_latency,
                     double* d_reliability, uint8_t* d_ok, void* stream) {
    if (!t || (q > 0 && (!d_pairs || !d_latency || !d_reliability || !d_ok))) return fail(SPE_EINVAL, "bad arguments");
    if (!t->built) return fail(SPE_ESTATE, "table not built");
    if (q == 0) return SPE_OK;
    return spe_lookup_batch_replica(t, 0, d_pairs, q, d_latency, d_reliability, d_ok, stream);
}

int spe_lookup_batch_replica(const spe_table* t, int32_t replica, const int32_t* d_pairs, int64_t q,
                             double* d_latency, double* d_reliability, uint8_t* d_ok, void* stream) {
    if (!t || (q > 0 && (!d_pairs || !d_latency || !d_reliability || !d_ok))) return fail(SPE_EINVAL, "bad arguments");
    if (!t->built) return fail(SPE_ESTATE, "table not built");
    if (q == 0) return SPE_OK;
    if (t->multi) return spe::multi_lookup(t->multi, replica, d_pairs, q, d_latency, d_reliability, d_ok, stream);
    if (replica != 0) return fail(SPE_EINVAL, "a single-device table has one replica (0)");
    HIP_TRY(hipSetDevice(t->g->device));
    hipStream_t s = stream ? (hipStream_t)stream : t->stream;
    k_lookup<1><<<grid_for(q, BLOCK, 16384), BLOCK, 0, s>>>((const int2*)d_pairs, q, t->blk0, t->blk1, t->tb,
                                                           d_latency, d_reliability, d_ok);
    HIP_TRY(hipGetLastError());
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPE_OK;
}

int spe_lookup_batch_host(const spe_table* t, const int32_t* pairs, int64_t q, double* latency, double* reliability,
                          uint8_t* ok) {
    if (!t || q < 0 || (q > 0 && (!pairs || !latency || !reliability || !ok))) return fail(SPE_EINVAL, "bad arguments");
    if (!t->built) return fail(SPE_ESTATE, "table not built");
    if (q == 0) return SPE_OK;
    int32_t dev = 0;
    if (int r = spe_table_replica_device(t, 0, &dev)) return r;
    spe_table::HostLookup* h = t->hlk;
    std::lock_guard<std::mutex> lock(h->mu);
    // chunks of up to 2M queries through two pinned staging slots: chunk k's pairs go up,
    // its lookups run and its answers come down on slot k % 2's stream while chunk k - 1's
    // answers are copied out (several threads: a host copy is the slowest leg)
    const int64_t chunk = std::min<int64_t>(q, (int64_t)1 << 21);
    if (int r = host_lookup_reserve(h, dev, chunk)) return r;
    const int64_t nch = (q + chunk - 1) / chunk;
    // on any error exit both slots' queued copies and lookups are drained first: they
    // write into the pinned staging a later call reuses (or host_lookup_reserve frees)
    struct Quiesce {
        spe_table::HostLookup* h;
        bool armed = true;
        ~Quiesce() {
            if (armed)
                for (int k = 0; k < 2; ++k)
                    if (h->sstream[k]) (void)hipStreamSynchronize(h->sstream[k]);
        }
    } quiesce{h};
    auto drain = [&](int64_t k) -> int {
        const int sl = (int)(k & 1);
        const int64_t i0 = k * chunk, n = std::min(chunk, q - i0);
        HIP_TRY(hipStreamSynchronize(h->sstream[sl]));
        pcopy(latency + i0, h->h_lat[sl], (size_t)n * sizeof(double));
        pcopy(reliability + i0, h->h_rel[sl], (size_t)n * sizeof(double));
        pcopy(ok + i0, h->h_ok[sl], (size_t)n);
        return SPE_OK;
    };
    for (int64_t k = 0; k < nch; ++k) {
        const int sl = (int)(k & 1);
        const int64_t i0 = k * chunk, n = std::min(chunk, q - i0);
        if (k >= 2)   // the slot's previous chunk must be out before its staging is reused
            if (int r = drain(k - 2)) return r;
        pcopy(h->h_pairs[sl], pairs + 2 * i0, (size_t)n * sizeof(int2));
        hipStream_t st = h->sstream[sl];
        HIP_TRY(hipMemcpyAsync(h->d_pairs[sl], h->h_pairs[sl], (size_t)n * sizeof(int2), hipMemcpyHostToDevice, st));
        if (int r = spe_lookup_batch_replica(t, 0, (const int32_t*)h->d_pairs[sl], n, h->d_lat[sl], h->d_rel[sl],
                                             h->d_ok[sl], st))
            return r;
        HIP_TRY(hipMemcpyAsync(h->h_lat[sl], h->d_lat[sl], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->h_rel[sl], h->d_rel[sl], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->h_ok[sl], h->d_ok[sl], (size_t)n, hipMemcpyDeviceToHost, st));
    }
    for (int64_t k = std::max<int64_t>(0, nch - 2); k < nch; ++k)
        if (int r = drain(k)) return r;
    quiesce.armed = false;
    return SPE_OK;
}

int spe_table_check(const spe_table* t, spe_check_report* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return fail(SPE_EUNSUPPORTED, "spe_table_check runs on single-device tables");
    if (t->blk0 != 0 || t->blk1 != (t->A + WAVE - 1) / WAVE) return fail(SPE_EUNSUPPORTED, "spe_table_check needs every source row");
    if (!t->built) return fail(SPE_ESTATE, "table not built");
    HIP_TRY(hipSetDevice(t->g->device));
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc(&d, 10 * sizeof(unsigned long long)));
    unsigned long long h[10];
    std::memset(h, 0, sizeof(h));
    h[9] = ~0ull;
    hipError_t e = hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice);
    // hop rule: per-source rows (no owner replay) of an undirected graph or a directed one alike
    const int32_t hop_rule = t->d_rank == nullptr;
    const int32_t undirected = !t->g->hg.directed && t->d_rank == nullptr;
    if (e == hipSuccess) {
        const int64_t total = (int64_t)((t->A + WAVE - 1) / WAVE) * t->A * WAVE;
        k_table_check<<<grid_for(total, BLOCK, 16384), BLOCK, 0, t->stream>>>(
            t->A, t->d_slot_vertex, t->d_vertex_slot, t->g->dev, undirected, hop_rule, t->tb, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SPE_EHIP, std::string("spe_table_check: ") + hipGetErrorString(e));
    out->pairs = (int64_t)h[0];
    out->unroutable = (int64_t)h[1];
    out->bad_values = (int64_t)h[2];
    out->next_not_adjacent = (int64_t)h[3];
    out->hop_checked = (int64_t)h[4];
    out->hop_mismatch = (int64_t)h[5];
    out->sym_checked = (int64_t)h[6];
    out->sym_mismatch = (int64_t)h[7];
    double w;
    std::memcpy(&w, &h[8], sizeof(w));
    out->max_sym_rel_err = w;
    out->first_bad_s = h[9] == ~0ull ? -1 : (int32_t)(h[9] >> 32);
    out->first_bad_t = h[9] == ~0ull ? -1 : (int32_t)(h[9] & 0xFFFFFFFFu);
    return SPE_OK;
}

int spe_table_compare(const spe_table* a, const spe_table* b, double rel_tol, spe_compare_report* out) {
    if (!a || !b || !out) return fail(SPE_EINVAL, "NULL argument");
    if (out->struct_size != sizeof(spe_compare_report)) return fail(SPE_EINVAL, ABI_MSG("spe_compare_report"));
    if (a->multi || b->multi) return fail(SPE_EUNSUPPORTED, "spe_table_compare runs on single-device tables");
    if (!a->built || !b->built) return fail(SPE_ESTATE, "table not built");
    if (a->g->device != b->g->device || a->A != b->A || a->blk0 != b->blk0 || a->blk1 != b->blk1 ||
        a->attached != b->attached)
        return fail(SPE_EINVAL, "spe_table_compare: the tables differ in device, attached slots or owned blocks");
    HIP_TRY(hipSetDevice(a->g->device));
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc(&d, 10 * sizeof(unsigned long long)));
    unsigned long long h[10];
    std::memset(h, 0, sizeof(h));
    h[9] = ~0ull;
    hipError_t e = hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice);
    // both tables' rows are complete once built; b's stream may still hold nothing
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) {
        const int64_t total = (int64_t)(a->blk1 - a->blk0) * a->A * WAVE;
        k_table_compare<<<grid_for(total, BLOCK, 16384), BLOCK, 0, a->stream>>>(a->A, a->blk0, total, a->tb, b->tb,
                                                                                rel_tol, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SPE_EHIP, std::string("spe_table_compare: ") + hipGetErrorString(e));
    out->pairs = (int64_t)h[0];
    out->routable = (int64_t)h[1];
    out->route_mismatch = (int64_t)h[2];
    out->latency_differs = (int64_t)h[3];
    out->reliability_differs = (int64_t)h[4];
    out->beyond_tolerance = (int64_t)h[5];
    out->delivery_flips = (int64_t)h[6];
    std::memcpy(&out->max_latency_rel_err, &h[7], sizeof(double));
    std::memcpy(&out->max_reliability_rel_err, &h[8], sizeof(double));
    out->first_bad_s = h[9] == ~0ull ? -1 : (int32_t)(h[9] >> 32);
    out->first_bad_t = h[9] == ~0ull ? -1 : (int32_t)(h[9] & 0xFFFFFFFFu);
    return SPE_OK;
}

int spe_table_replica_device(const spe_table* t, int32_t replica, int32_t* device) {
    if (!t || !device) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return spe::multi_replica_device(t->multi, replica, device);
    if (replica != 0) return fail(SPE_EINVAL, "a single-device table has one replica (0)");
    *device = t->g->device;
    return SPE_OK;
}

int spe_table_digest(const spe_table* t, int32_t block_begin, int32_t block_end, spe_block_digest* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return spe_table_digest_replica(t, 0, block_begin, block_end, out);
    return spe::table_digest_fields(t, block_begin, block_end, 15u, out);
}

int spe_table_digest_replica(const spe_table* t, int32_t replica, int32_t block_begin, int32_t block_end,
                             spe_block_digest* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) {
        if (!t->built) return fail(SPE_ESTATE, "table not built");
        return spe::multi_digest(t->multi, replica, block_begin, block_end, out);
    }
    if (replica != 0) return fail(SPE_EINVAL, "a single-device table has one replica (0)");
    return spe::table_digest_fields(t, block_begin, block_end, 15u, out);
}

int spe_table_replica_latrel(const spe_table* t, int32_t replica, void** latrel) {
    if (!t || !latrel) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return spe::multi_replica_latrel(t->multi, replica, latrel);
    if (replica != 0) return fail(SPE_EINVAL, "a single-device table has one replica (0)");
    *latrel = t->tb.lr;
    return SPE_OK;
}

int spe_table_verify_replicas(const spe_table* t, spe_replica_report* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (out->struct_size != sizeof(spe_replica_report)) return fail(SPE_EINVAL, ABI_MSG("spe_replica_report"));
    if (!t->built) return fail(SPE_ESTATE, "table not built");
    if (t->multi) return spe::multi_verify(t->multi, out);
    out->replicas = 1;
    out->blocks = t->blk1 - t->blk0;
    out->mismatching_blocks = 0;
    out->first_bad_replica = out->first_bad_block = -1;
    out->seconds = 0.0;
    return SPE_OK;
}

}  // extern "C"

int spe::digest_span(int32_t device, void* stream, int32_t A, int32_t b0, int32_t nb, const void* latrel,
                     const void* next_hop, const void* hops, uint32_t fields, uint64_t* d_out) {
    uint32_t mask = fields & 15u;
    if (!latrel) mask &= ~3u;
    if (!next_hop) mask &= ~4u;
    if (!hops) mask &= ~8u;
    if (nb <= 0 || !mask) return SPE_OK;
    HIP_TRY(hipSetDevice(device));
    // one wave per (block, DG_TC targets) item; 2048 workgroups = every wave slot of the
    // device (256 CUs x 32 waves), larger tables take further grid-stride passes
    const int64_t items = (int64_t)nb * ((A + DG_TC - 1) / DG_TC);
    k_table_digest<<<grid_for(items * WAVE, BLOCK, 2048), BLOCK, 0, (hipStream_t)stream>>>(
        A, b0, nb, (const double2*)latrel, (const int32_t*)next_hop, (const uint16_t*)hops, mask,
        (unsigned long long*)d_out);
    HIP_TRY(hipGetLastError());
    return SPE_OK;
}

int spe::table_digest_fields(const spe_table* t, int32_t block_begin, int32_t block_end, uint32_t fields,
                             spe_block_digest* out) {
    if (!t || !out || t->multi) return fail(SPE_EINVAL, "NULL argument");
    if (block_begin < t->blk0 || block_end > t->blk1 || block_begin >= block_end)
        return fail(SPE_EINVAL, "block range empty, reversed or not owned by this table");
    for (int32_t b = block_begin; b < block_end; ++b)
        if (!t->blk_built[(size_t)(b - t->blk0)]) return fail(SPE_ESTATE, "blocks not built");
    static_assert(sizeof(spe_block_digest) == 4 * sizeof(uint64_t), "spe_block_digest is the kernel's out[block][4]");
    HIP_TRY(hipSetDevice(t->g->device));
    const int32_t nb = block_end - block_begin;
    const size_t bytes = (size_t)nb * sizeof(spe_block_digest);
    uint64_t* d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    const size_t off = (size_t)(block_begin - t->blk0) * t->A * WAVE;
    hipError_t e = hipMemsetAsync(d, 0, bytes, t->stream);
    int r = SPE_OK;
    if (e == hipSuccess)
        r = spe::digest_span(t->g->device, t->stream, t->A, block_begin, nb, t->tb.lr + off, t->tb.next + off,
                             t->tb.hops + off, fields, d);
    if (e == hipSuccess && !r) e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, t->stream);
    const hipError_t es = hipStreamSynchronize(t->stream);   // also on an error: nothing may still write d
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (r) return r;
    if (e != hipSuccess) return fail(SPE_EHIP, std::string("spe_table_digest: ") + hipGetErrorString(e));
    return SPE_OK;
}

int spe::lookup_on_replica(int32_t device, const void* latrel, int32_t A, int32_t nblk, const int32_t* d_pairs,
                           int64_t q, double* d_latency, double* d_reliability, uint8_t* d_ok, void* stream) {
    HIP_TRY(hipSetDevice(device));
    Table tb{};
    tb.lr = (double2*)latrel;
    tb.A = A;
    hipStream_t s = (hipStream_t)stream;
    k_lookup<1><<<grid_for(q, BLOCK, 16384), BLOCK, 0, s>>>((const int2*)d_pairs, q, 0, nblk, tb, d_latency,
                                                           d_reliability, d_ok);
    HIP_TRY(hipGetLastError());
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPE_OK;
}

extern "C" {

int spe_fw_apsp(spe_graph* g, double* d_dist, int64_t ld, int32_t* d_next, void* stream, double* seconds) {
    if (!g || !d_dist) return fail(SPE_EINVAL, "NULL argument");
    const int32_t n = g->hg.nc;
    const int32_t nb = (n + FWB - 1) / FWB;
    if (ld < (int64_t)nb * FWB) return fail(SPE_EINVAL, "ld must be >= the relaxation vertex count rounded up to 64");
    if (ld % FWB) return fail(SPE_EINVAL, "ld must be a multiple of 64");
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, s));
    k_fw_init<<<grid_for(ld * ld, 256, 16384), 256, 0, s>>>(n, ld, g->dev, d_dist);
    const int32_t nrel = (int32_t)g->hg.icol.size();
    if (nrel > 0) k_fw_edges<<<(nrel + 255) / 256, 256, 0, s>>>(nrel, ld, g->dev, d_dist);
    // padding rows / columns stay +inf off the diagonal: they never shorten a path
    for (int32_t kb = 0; kb < nb; ++kb) {
        k_fw_panel<<<1, 256, 0, s>>>(kb, nb, ld, d_dist, 0);
        if (nb > 1) k_fw_panel<<<2 * nb - 2, 256, 0, s>>>(kb, nb, ld, d_dist, 1);
        if (nb > 1) k_fw_rest<<<(nb - 1) * (nb - 1), 256, 0, s>>>(kb, nb, ld, d_dist);
    }
    HIP_TRY(hipEventRecord(b, s));
    if (d_next) k_fw_next<<<grid_for((int64_t)n * n, 256, 16384), 256, 0, s>>>(n, ld, g->dev, d_dist, d_next);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    if (seconds) *seconds = ms / 1e3;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return SPE_OK;
}

namespace {
__global__ __launch_bounds__(256) void k_fw3_first_hop(int64_t total, const int32_t* __restrict__ irow,
                                                       int32_t* __restrict__ nxt) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int32_t k = nxt[e];
        nxt[e] = k < 0 ? -1 : irow[k];
    }
}
}  // namespace

int spe_fw_closure(spe_graph* g, double* d_dist, double* d_rel, int32_t* d_next, int64_t ld, void* stream,
                   double* seconds) {
    if (!g || !d_dist || !d_next) return fail(SPE_EINVAL, "NULL argument");   // d_rel NULL: the (D, N) pair
    const int32_t n = g->hg.nc;
    if (ld < ((int64_t)n + FWB - 1) / FWB * FWB || ld % FWB) return fail(SPE_EINVAL, "ld must be a multiple of 64 >= n");
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, s));
    if (int r = fw3_closure(g, Fw3{d_dist, d_rel, d_next}, ld, s)) return r;
    HIP_TRY(hipEventRecord(b, s));
    k_fw3_first_hop<<<grid_for(ld * ld, 256, 16384), 256, 0, s>>>(ld * ld, g->dev.irow, d_next);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    if (seconds) *seconds = ms / 1e3;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return SPE_OK;
}

int spe_table_source_tree(spe_table* t, int32_t s_slot, int32_t* parent) {
    if (!t || !parent) return fail(SPE_EINVAL, "NULL argument");
    if (t->multi) return spe::multi_source_tree(t->multi, s_slot, parent);
    if (s_slot < 0 || s_slot >= t->A) return fail(SPE_EINVAL, "slot out of range");
    const int32_t b = s_slot / WAVE;
    if (b < t->blk0 || b >= t->blk1) return fail(SPE_EINVAL, "source block not owned by this table");
    if (t->md.complete) return fail(SPE_EUNSUPPORTED, "DIRECT table: every path is its one edge");
    // owner replay rewrites pairs across blocks (k_owner_replay): rebuilding one block would undo it
    if (t->d_rank) return fail(SPE_EUNSUPPORTED, "owner-replay table: its entries are not one source's tree");
    const spe::HostGraph& h = t->g->hg;
    const int32_t nc = h.nc, s = t->attached[(size_t)s_slot];
    // pk[v]: in-CSR entry of the relaxation vertex v's parent edge; -1 none (root or
    // unreached); -2 (batch / FW state) the pruned pendant source itself
    std::vector<int32_t> pk((size_t)std::max(1, nc), -1);
    HIP_TRY(hipSetDevice(t->g->device));
    // The source is re-run into scratch rows of one block, never into the table itself:
    // concurrent readers of a live table (the topology shim's queries) keep seeing its
    // finished rows (a prefer-direct row would otherwise lack the DIRECT overlay for a while).
    const size_t be = (size_t)t->A * WAVE;
    const bool scratch = !t->tb.prev && !t->tb.aux;   // aux tables (offline tool only) rebuild in place
    void* sbuf = nullptr;
    if (scratch) HIP_TRY(hipMalloc(&sbuf, be * (sizeof(double2) + sizeof(int32_t) + sizeof(uint16_t))));
    double2* s_lr = (double2*)sbuf;
    int32_t* s_next = (int32_t*)(s_lr + (scratch ? be : 0));
    uint16_t* s_hops = (uint16_t*)(s_next + (scratch ? be : 0));
    int rc = SPE_OK;
    if (t->engine == SPE_ENGINE_LDS) {
        // one workgroup re-runs this source; the parent entries stay in that workgroup's scratch
        Table tb = t->tb;
        int32_t blk0 = t->blk0;
        if (scratch) {
            tb.lr = s_lr;
            tb.next = s_next;
            tb.hops = s_hops;
            blk0 = b;   // the scratch holds block b only
        }
        k_sssp_lds<<<1, LDS_T, lds_bytes(nc), t->stream>>>(s_slot, s_slot + 1, t->d_slots, blk0, t->g->dev, t->md, tb,
                                                         t->lsc, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(pk.data(), t->lsc.par, sizeof(int32_t) * (size_t)nc,
                                                hipMemcpyDeviceToHost, t->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
        if (e != hipSuccess) rc = fail(SPE_EHIP, hipGetErrorString(e));
        // in place (aux tables): the row just rewritten lacks the DIRECT overlay; rebuild the block
        if (!rc && !scratch && t->md.prefer) rc = spe_table_build_blocks(t, b, b + 1, nullptr);
    } else {
        // re-run the source's block, one lane per source (no shared anchor trees); its
        // state is left in the first buffer
        t->share_off = true;
        rc = scratch ? spe_table_build_blocks_into(t, b, b + 1, s_lr, s_next, s_hops, nullptr)
                     : spe_table_build_blocks(t, b, b + 1, nullptr);
        t->share_off = false;
        if (!rc) {
            const hipError_t e = hipStreamSynchronize(t->stream);
            if (e != hipSuccess) rc = fail(SPE_EHIP, hipGetErrorString(e));
        }
    }
    if (sbuf) (void)hipFree(sbuf);
    if (rc) return rc;
    if (t->engine != SPE_ENGINE_LDS && t->cx) {
        // the contracted graph: kept rows carry entries of the contracted CSR (a shortcut
        // entry's parent is its x); a removed vertex's parent is the best of its three
        // neighbours, the rows kernel's rule
        const spe::HostGraph::Contracted& cx = h.cx;
        const int32_t nk = cx.nk, L = t->lanes, j = s_slot % WAVE;
        const int32_t g = L <= WAVE ? j / L : 0, lane = L <= WAVE ? j % L : j;
        std::vector<int32_t> kp((size_t)std::max(1, nk));
        std::vector<double> kd((size_t)std::max(1, nk));
        const size_t off = ((size_t)g * nk) * (size_t)L + (size_t)lane;
        HIP_TRY(hipMemcpy2D(kp.data(), sizeof(int32_t), t->st_buf[0].P + off, sizeof(int32_t) * (size_t)L,
                            sizeof(int32_t), (size_t)nk, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(kd.data(), sizeof(double), t->st_buf[0].D + off, sizeof(double) * (size_t)L,
                            sizeof(double), (size_t)nk, hipMemcpyDeviceToHost));
        std::fill(parent, parent + h.n, -1);
        auto orig = [&](int32_t kv) { return h.corev[(size_t)cx.kcore[(size_t)kv]]; };
        for (int32_t v = 0; v < nk; ++v) {
            const int32_t k = kp[(size_t)v];
            if (k >= 0) parent[orig(v)] = cx.via[(size_t)k] >= 0 ? cx.via[(size_t)k] : orig(cx.col[(size_t)k]);
            else if (k == -2) parent[orig(v)] = s;   // the source's first edge (pendant or contracted source)
        }
        for (size_t r = 0; r < cx.rcore.size(); ++r) {
            const int32_t x = h.corev[(size_t)cx.rcore[r]];
            if (x == s) continue;
            int32_t bq = -1;
            double bd = INF, bdu = INF;
            for (int q = 0; q < 3; ++q) {
                const double du = kd[(size_t)cx.rnb[3 * r + q]];
                if (!(du < INF)) continue;
                const double alt = du + cx.rw[3 * r + q];
                if (bq < 0 || alt < bd || (alt == bd && du < bdu)) {
                    bq = q;
                    bd = alt;
                    bdu = du;
                }
            }
            if (bq >= 0) parent[x] = orig(cx.rnb[3 * r + bq]);
        }
        if (h.pruned)
            for (int32_t v = 0; v < h.n; ++v) {
                if (h.core_id[(size_t)v] >= 0 || v == s) continue;
                const int32_t a = h.anchor_core[(size_t)v];   // (never a removed vertex)
                if (a >= 0 && kd[(size_t)cx.kid[(size_t)a]] < INF) parent[v] = h.corev[(size_t)a];
            }
        parent[s] = -1;
        return SPE_OK;
    }
    if (t->engine != SPE_ENGINE_LDS) {
        const int32_t L = t->lanes, j = s_slot % WAVE;
        const int32_t g = L <= WAVE ? j / L : 0, lane = L <= WAVE ? j % L : j;
        const int32_t* P = t->st_buf[0].P + ((size_t)g * nc) * (size_t)L + (size_t)lane;
        HIP_TRY(hipMemcpy2D(pk.data(), sizeof(int32_t), P, sizeof(int32_t) * (size_t)L, sizeof(int32_t), (size_t)nc,
                            hipMemcpyDeviceToHost));
    }
    std::fill(parent, parent + h.n, -1);
    const int32_t sc = h.core_id[(size_t)s];
    const int32_t root = sc >= 0 ? sc : h.anchor_core[(size_t)s];   // relaxation vertex the tree grows from
    std::vector<uint8_t> reach((size_t)std::max(1, nc), 0);
    for (int32_t v = 0; v < nc; ++v) {
        const int32_t k = pk[(size_t)v];
        if (k >= 0) {
            parent[h.corev[(size_t)v]] = h.corev[(size_t)h.icol[(size_t)k]];
            reach[(size_t)v] = 1;
        } else if (v == root) {
            if (sc < 0) parent[h.corev[(size_t)v]] = s;   // s -> anchor: the pendant source's edge
            reach[(size_t)v] = 1;
        }
    }
    if (h.pruned)
        for (int32_t v = 0; v < h.n; ++v) {
            if (h.core_id[(size_t)v] >= 0 || v == s) continue;
            const int32_t a = h.anchor_core[(size_t)v];
            if (a >= 0 && reach[(size_t)a]) parent[v] = h.corev[(size_t)a];
        }
    parent[s] = -1;
    return SPE_OK;
}

int spe_table_min_latency(const spe_table* t, double* out) {
    if (!t || !out) return fail(SPE_EINVAL, "NULL argument");
    if (!t->built) return fail(SPE_ESTATE, "table not built (every owned block)");
    if (t->multi) return spe::multi_min_latency(t->multi, out);
    HIP_TRY(hipSetDevice(t->g->device));
    const unsigned long long init = 0x7FF0000000000000ull;  // +inf
    HIP_TRY(hipMemcpyAsync(t->d_min, &init, sizeof(init), hipMemcpyHostToDevice, t->stream));
    const int64_t elems = (int64_t)(t->blk1 - t->blk0) * t->A * WAVE;
    k_min_latency<<<grid_for(elems, BLOCK, 4096), BLOCK, 0, t->stream>>>(t->tb.lr, elems, t->A, t->blk0,
                                                                        t->d_min);
    HIP_TRY(hipGetLastError());
    unsigned long long bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, t->d_min, sizeof(bits), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    double v;
    std::memcpy(&v, &bits, sizeof(v));
    *out = (v == INF) ? 0.0 : v;   // reference's "0 = unset" sentinel, shd-topology.c:1360
    return SPE_OK;
}

// ---------------------------------------------------------------- table cache
// File: 64-byte header, then the owned SB64 span of each field (latrel, next,
// hops), raw.  Written to "<path>.tmp" and renamed, so a reader never sees a
// partial file under the final name.
namespace {
struct CacheHeader {
    char magic[8];        // "SPETAB01"
    uint64_t key;
    int32_t A, blk0, blk1, pad;
    int64_t elems;
    int64_t bytes;        // payload bytes after the header
    char reserved[16];
};
static_assert(sizeof(CacheHeader) == 64, "cache header is 64 bytes");
const char kMagic[8] = {'S', 'P', 'E', 'T', 'A', 'B', '0', '1'};
constexpr size_t kChunk = 64u << 20;   // staging chunk

struct Field {
    void* dev;
    size_t bytes;
};

void fields_of(const spe_table* t, Field f[3], int64_t* elems) {
    const int64_t e = (int64_t)(t->blk1 - t->blk0) * t->A * WAVE;
    *elems = e;
    f[0] = {t->tb.lr, (size_t)e * sizeof(double2)};
    f[1] = {t->tb.next, (size_t)e * sizeof(int32_t)};
    f[2] = {t->tb.hops, (size_t)e * sizeof(uint16_t)};
}
}  // namespace

int spe_table_key(const spe_table* t, uint64_t* key) {
    if (!t || !key) return fail(SPE_EINVAL, "NULL argument");
    *key = t->key;
    return SPE_OK;
}

int spe_table_save(const spe_table* t, const char* path) {
    if (t && t->tb.aux) return fail(SPE_EUNSUPPORTED, "the table cache does not hold want_aux rows");
    if (t && t->multi) return fail(SPE_EUNSUPPORTED, "the table cache holds single-device tables");
    if (!t || !path) return fail(SPE_EINVAL, "NULL argument");
    if (!t->built) return fail(SPE_ESTATE, "table not built (every owned block)");
    HIP_TRY(hipSetDevice(t->g->device));
    HIP_TRY(hipStreamSynchronize(t->stream));
    Field f[3];
    int64_t elems = 0;
    fields_of(t, f, &elems);
    CacheHeader h{};
    std::memcpy(h.magic, kMagic, 8);
    h.key = t->key;
    h.A = t->A;
    h.blk0 = t->blk0;
    h.blk1 = t->blk1;
    h.elems = elems;
    h.bytes = (int64_t)(f[0].bytes + f[1].bytes + f[2].bytes);
    const std::string tmp = std::string(path) + ".tmp";
    FILE* fp = fopen(tmp.c_str(), "wb");
    if (!fp) return fail(SPE_EINVAL, "cannot create " + tmp);
    void* stage = nullptr;
    if (hipHostMalloc(&stage, kChunk) != hipSuccess) {
        fclose(fp);
        remove(tmp.c_str());
        return fail(SPE_ENOMEM, "cache staging buffer");
    }
    int rc = SPE_OK;
    if (fwrite(&h, sizeof(h), 1, fp) != 1) rc = fail(SPE_EINVAL, "short write " + tmp);
    for (int i = 0; i < 3 && rc == SPE_OK; ++i) {
        for (size_t off = 0; off < f[i].bytes && rc == SPE_OK; off += kChunk) {
            const size_t n = std::min(kChunk, f[i].bytes - off);
            const hipError_t e = hipMemcpy(stage, (const char*)f[i].dev + off, n, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(SPE_EHIP, std::string("hipMemcpy D2H: ") + hipGetErrorString(e));
            else if (fwrite(stage, 1, n, fp) != n) rc = fail(SPE_EINVAL, "short write " + tmp);
        }
    }
    (void)hipHostFree(stage);
    if (fclose(fp) != 0 && rc == SPE_OK) rc = fail(SPE_EINVAL, "close " + tmp);
    if (rc == SPE_OK && rename(tmp.c_str(), path) != 0) rc = fail(SPE_EINVAL, std::string("rename to ") + path);
    if (rc != SPE_OK) remove(tmp.c_str());
    return rc;
}

int spe_table_load(spe_table* t, const char* path) {
    if (t && t->tb.aux) return fail(SPE_EUNSUPPORTED, "the table cache does not hold want_aux rows");
    if (t && t->multi) return fail(SPE_EUNSUPPORTED, "the table cache holds single-device tables");
    if (!t || !path) return fail(SPE_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(t->g->device));
    FILE* fp = fopen(path, "rb");
    if (!fp) return fail(SPE_EINVAL, std::string("no cache file ") + path);
    Field f[3];
    int64_t elems = 0;
    fields_of(t, f, &elems);
    CacheHeader h{};
    int rc = SPE_OK;
    if (fread(&h, sizeof(h), 1, fp) != 1 || std::memcmp(h.magic, kMagic, 8) != 0)
        rc = fail(SPE_EINVAL, std::string("not a path-table cache: ") + path);
    else if (h.key != t->key || h.A != t->A || h.blk0 != t->blk0 || h.blk1 != t->blk1 || h.elems != elems ||
             h.bytes != (int64_t)(f[0].bytes + f[1].bytes + f[2].bytes))
        rc = fail(SPE_EINVAL, std::string("cache file is for another graph / attached set / options: ") + path);
    void* stage = nullptr;
    if (rc == SPE_OK && hipHostMalloc(&stage, kChunk) != hipSuccess) rc = fail(SPE_ENOMEM, "cache staging buffer");
    for (int i = 0; i < 3 && rc == SPE_OK; ++i) {
        for (size_t off = 0; off < f[i].bytes && rc == SPE_OK; off += kChunk) {
            const size_t n = std::min(kChunk, f[i].bytes - off);
            if (fread(stage, 1, n, fp) != n) {
                rc = fail(SPE_EINVAL, std::string("truncated cache file ") + path);
                break;
            }
            const hipError_t e = hipMemcpy((char*)f[i].dev + off, stage, n, hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = fail(SPE_EHIP, std::string("hipMemcpy H2D: ") + hipGetErrorString(e));
        }
    }
    if (stage) (void)hipHostFree(stage);
    fclose(fp);
    if (rc == SPE_OK) {
        t->built = true;
        std::fill(t->blk_built.begin(), t->blk_built.end(), (uint8_t)1);
    }
    return rc;
}

static void host_lookup_free(spe_table::HostLookup* h) {
    if (!h) return;
    if (h->device >= 0) {
        (void)hipSetDevice(h->device);
        for (int k = 0; k < 2; ++k) {
            if (h->sstream[k]) (void)hipStreamSynchronize(h->sstream[k]);
            for (void* p : {(void*)h->d_pairs[k], (void*)h->d_lat[k], (void*)h->d_rel[k], (void*)h->d_ok[k]})
                if (p) (void)hipFree(p);
            for (void* p : {(void*)h->h_pairs[k], (void*)h->h_lat[k], (void*)h->h_rel[k], (void*)h->h_ok[k]})
                if (p) (void)hipHostFree(p);
            if (h->sstream[k]) (void)hipStreamDestroy(h->sstream[k]);
        }
        if (h->h_entry) (void)hipHostFree(h->h_entry);
        if (h->d_row) (void)hipFree(h->d_row);
        if (h->h_row) (void)hipHostFree(h->h_row);
    }
    delete h;
}

void spe_table_free(spe_table* t) {
    if (!t) return;
    host_lookup_free(t->hlk);
    t->hlk = nullptr;
    if (t->multi) {
        spe::multi_free(t->multi);
        delete t;
        return;
    }
    host_prefault_stop(t);   // before the mapping goes
    (void)hipSetDevice(t->g->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    for (void* p : t->allocs) (void)hipFree(p);
    if (t->h_srcv) (void)hipHostFree(t->h_srcv);
    if (t->h_rows) (void)hipHostFree(t->h_rows);
    if (t->h_unsafe) (void)hipHostFree(t->h_unsafe);
    if (t->h_der) (void)hipHostFree(t->h_der);
    if (t->h_sunsafe) (void)hipHostFree(t->h_sunsafe);
    if (t->h_counts) (void)hipHostFree(t->h_counts);
    for (hipEvent_t e : t->ev_pool) (void)hipEventDestroy(e);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    if (t->rows_stream) (void)hipStreamDestroy(t->rows_stream);
    if (t->ev_relaxed) (void)hipEventDestroy(t->ev_relaxed);
    for (hipEvent_t e : t->ev_rows)
        if (e) (void)hipEventDestroy(e);
    if (t->h_dl) (void)hipHostFree(t->h_dl);
    for (hipEvent_t e : t->ev_dl)
        if (e) (void)hipEventDestroy(e);
    delete t;
}

int spe_delivery_near_boundary(double latency_ms, int32_t hops) { return delivery_near_boundary(latency_ms, hops) ? 1 : 0; }

}  // extern "C"

