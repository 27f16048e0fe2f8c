// ffi.cpp — C-ABI implementation of libspectre_gpu.so (see
// include/spectre_gpu.h for the boundary contract and INTEGRATION.md for the
// Rust-side binding that slots this beneath halo2's best_multiexp/best_fft).
//
// Host-side work is deliberately tiny: context/stream/cache management,
// SRS upload caching, and the final window-Horner (<= 256 point ops per MSM)
// + one field inversion to normalize to affine. All bulk compute runs in the
// HIP kernels (msm.hip / ntt.hip); there is no CPU fallback path.
#include "internal.hpp"
#include "spectre_gpu.h"
#include <cstdarg>
#include <cstdlib>
#include <cstdio>

thread_local std::string g_last_error;
void set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

extern "C" {

const char* spectre_gpu_last_error(void) { return g_last_error.c_str(); }
const char* spectre_gpu_version(void) { return "spectre-amd 0.1.0 gfx950"; }

spectre_gpu_ctx* spectre_gpu_init(int device_count, const int* device_ids) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_err("spectre_gpu_init: no visible HIP devices (this library has "
                "no CPU fallback by design)");
        return nullptr;
    }
    if (device_count <= 0) device_count = 1;
    auto* ctx = new spectre_gpu_ctx();
    for (int i = 0; i < device_count; i++) {
        int id = device_ids ? device_ids[i] : i;
        if (id < 0 || id >= ndev) {
            set_err("spectre_gpu_init: device id %d out of range (%d devices)",
                    id, ndev);
            delete ctx;
            return nullptr;
        }
        DeviceState ds;
        ds.device_id = id;
        if (hipSetDevice(id) != hipSuccess ||
            hipStreamCreate(&ds.stream) != hipSuccess) {
            set_err("spectre_gpu_init: failed to init device %d", id);
            delete ctx;
            return nullptr;
        }
        ctx->devs.push_back(ds);
    }
    // SPECTRE_MSM_ACC_E presets the entries per accumulate thread (tuning
    // A/B from tools that do not call the setter); unusable values = auto
    if (const char* e = getenv("SPECTRE_MSM_ACC_E")) {
        const long v = atol(e);
        if (v > 0 && !(v & 3) && v <= (long)SPECTRE_MSM_ACC_ENTRIES_MAX)
            ctx->msm_acc_entries = (uint32_t)v;
    }
    // SPECTRE_NTT_FORCE3 (any value) takes the three-axis NTT split at sizes
    // that do not need it, where the oracle can check it; read once so the
    // cached plans of a context all follow one rule
    ctx->ntt_force3 = getenv("SPECTRE_NTT_FORCE3") != nullptr;
    return ctx;
}

void spectre_gpu_destroy(spectre_gpu_ctx* ctx) {
    if (!ctx) return;
    for (auto& ds : ctx->devs) {
        (void)hipSetDevice(ds.device_id);
        ds.release();
    }
    delete ctx;
}

int spectre_gpu_device_count(spectre_gpu_ctx* ctx) {
    return ctx ? (int)ctx->devs.size() : 0;
}

int spectre_gpu_set_msm_acc_entries(spectre_gpu_ctx* ctx, uint32_t e) {
    if (!ctx || (e & 3) || e > SPECTRE_MSM_ACC_ENTRIES_MAX) {
        set_err("set_msm_acc_entries: %u is not 0 or a multiple of 4 <= %u",
                e, SPECTRE_MSM_ACC_ENTRIES_MAX);
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->msm_acc_entries = e;
    return 0;
}

uint32_t spectre_gpu_msm_acc_auto_entries(uint64_t entries, uint32_t cus,
                                          uint32_t resident_blocks) {
    return msm_acc_auto_entries(entries, cus, resident_blocks);
}

int spectre_gpu_msm_fold_window(const uint8_t p0[96], const uint8_t p1[96],
                                const uint8_t p2[96], uint8_t out[96]) {
    if (!p0 || !p1 || !p2 || !out) {
        set_err("msm_fold_window: null argument");
        return -1;
    }
    g1_jac p[3], sum;
    memcpy(&p[0], p0, 96);
    memcpy(&p[1], p1, 96);
    memcpy(&p[2], p2, 96);
    msm_fold_window(p[0], p[1], p[2], sum);
    memcpy(out, &sum, 96);
    return 0;
}

// ---------------------------------------------------------------- staging
#define STAGE_CHUNK (16u << 20)

static int ensure_stage(DeviceState& ds) {
    for (int b = 0; b < 2; b++) {
        RC_TRY(ds.h_stage[b].reserve(STAGE_CHUNK));
        if (ds.stage_ev[b]) continue;
        HIP_TRY(hipEventCreate(&ds.stage_ev[b]));
        HIP_TRY(hipEventRecord(ds.stage_ev[b], ds.stream));
    }
    return 0;
}

// host->device on ds.stream through alternating pinned chunks: pageable
// hipMemcpy runs at ~3 GB/s; here the memcpy of chunk k+1 overlaps the DMA
// of chunk k, which reaches ~3-4x that. The stream stays ordered, so
// following kernels need no extra sync, and the user buffer is fully
// consumed by the memcpys before return (the in-flight DMA reads only
// pinned memory).
static int staged_upload(DeviceState& ds, void* d_dst, const void* src,
                         size_t bytes) {
    RC_TRY(ensure_stage(ds));
    size_t off = 0;
    int b = 0;
    while (off < bytes) {
        const size_t len = bytes - off < STAGE_CHUNK ? bytes - off : STAGE_CHUNK;
        HIP_TRY(hipEventSynchronize(ds.stage_ev[b]));  // buffer free?
        memcpy(ds.h_stage[b].ptr, (const uint8_t*)src + off, len);
        HIP_TRY(hipMemcpyAsync((uint8_t*)d_dst + off, ds.h_stage[b].ptr, len,
                               hipMemcpyHostToDevice, ds.stream));
        HIP_TRY(hipEventRecord(ds.stage_ev[b], ds.stream));
        off += len;
        b ^= 1;
    }
    return 0;
}

static int staged_download(DeviceState& ds, void* dst, const void* d_src,
                           size_t bytes) {
    RC_TRY(ensure_stage(ds));
    size_t off = 0;
    int b = 0;
    size_t pend_off[2] = {0, 0}, pend_len[2] = {0, 0};
    while (off < bytes) {
        const size_t len = bytes - off < STAGE_CHUNK ? bytes - off : STAGE_CHUNK;
        if (pend_len[b]) {  // drain the older use of this buffer
            HIP_TRY(hipEventSynchronize(ds.stage_ev[b]));
            memcpy((uint8_t*)dst + pend_off[b], ds.h_stage[b].ptr,
                   pend_len[b]);
        }
        HIP_TRY(hipMemcpyAsync(ds.h_stage[b].ptr, (const uint8_t*)d_src + off,
                               len, hipMemcpyDeviceToHost, ds.stream));
        HIP_TRY(hipEventRecord(ds.stage_ev[b], ds.stream));
        pend_off[b] = off;
        pend_len[b] = len;
        off += len;
        b ^= 1;
    }
    for (int i = 0; i < 2; i++) {
        if (pend_len[i]) {
            HIP_TRY(hipEventSynchronize(ds.stage_ev[i]));
            memcpy((uint8_t*)dst + pend_off[i], ds.h_stage[i].ptr,
                   pend_len[i]);
        }
    }
    return 0;
}

// ---------------------------------------------------------------- helpers
static int check_dev(spectre_gpu_ctx* ctx, int dev) {
    if (!ctx || dev < 0 || dev >= (int)ctx->devs.size()) {
        set_err("invalid ctx/device index %d", dev);
        return -1;
    }
    return 0;
}

// A batched MSM sizes host memory by nbatch, so the bound that the MSM itself
// applies (msm_acquire_slot) is checked before anything is sized.
static int check_nbatch(uint32_t nbatch) {
    if (nbatch == 0 || nbatch > SPECTRE_MSM_MAX_BATCH) {
        set_err("msm: nbatch %u out of range [1,%d]", nbatch,
                SPECTRE_MSM_MAX_BATCH);
        return -3;
    }
    return 0;
}

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?
static bool ranges_overlap(const void* a, uint64_t a_bytes, const void* b,
                           uint64_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes &&
           (uintptr_t)b < (uintptr_t)a + a_bytes;
}

// the element at `bytes`, or one where the caller passed NULL
static fp256 fr_or_one(const uint8_t* bytes) {
    fp256 v;
    if (bytes) ff_from_bytes(v, bytes);
    else ff_set_one<Fr>(v);
    return v;
}

// Horner over the 16 windows + normalize to affine (host; <=256 point ops).
static void winsums_to_affine(const g1_jac* wins, uint8_t out[64]) {
    g1_jac res;
    g1j_set_inf(res);
    for (int w = MSM_NWIN - 1; w >= 0; w--) {
        if (w != MSM_NWIN - 1) {
            for (int d = 0; d < MSM_WBITS; d++) g1j_dbl_ip(res);
        }
        g1j_add_ip(res, wins[w]);
    }
    g1_affine a;
    g1j_to_affine(a, res);
    ff_to_bytes(out, a.x);
    ff_to_bytes(out + 32, a.y);
}

int spectre_gpu_msm_g1_combine(const uint8_t* partials, uint32_t nshards,
                               uint8_t out_affine[64]) {
    if (!partials || nshards == 0) {
        set_err("combine: bad args");
        return -1;
    }
    g1_jac tot[MSM_NWIN];
    for (int w = 0; w < MSM_NWIN; w++) g1j_set_inf(tot[w]);
    for (uint32_t s = 0; s < nshards; s++) {  // deterministic rank order
        const g1_jac* sh = (const g1_jac*)(partials + (size_t)s * MSM_NWIN * 96);
        for (int w = 0; w < MSM_NWIN; w++) g1j_add_ip(tot[w], sh[w]);
    }
    winsums_to_affine(tot, out_affine);
    return 0;
}

// ---------------------------------------------------------------- MSM
// a full-window-range call description
static MsmCall msm_call(const void* d_bases, const void* d_scalars,
                        uint32_t nbatch, uint64_t n, uint32_t flags) {
    return {(const g1_affine*)d_bases, (const uint8_t*)d_scalars, nbatch, n,
            flags, 0, MSM_NWIN};
}

// Round-robin slot for the async entry points. Measured on MI355X (r2):
// depth 3 = 325.6 MSM(2^20)/s vs depth 2 = 300 vs unpipelined = 240 — three
// in flight keep the machine fed through each call's host-combine + sync
// gap, so every slot is used unless SPECTRE_PIPE_SLOTS asks for fewer.
static int next_async_slot(DeviceState& ds) {
    static const int kSlots = []() {
        const char* e = getenv("SPECTRE_PIPE_SLOTS");
        const int v = e ? atoi(e) : MSM_SLOTS;
        return v < 1 ? 1 : (v > MSM_SLOTS ? MSM_SLOTS : v);
    }();
    const int slot = ds.next_slot;
    ds.next_slot = (slot + 1) % kSlots;
    return slot;
}

int spectre_gpu_msm_g1_shard_device(spectre_gpu_ctx* ctx, int dev,
                                    const void* d_bases, const void* d_scalars,
                                    uint64_t n, uint32_t flags,
                                    uint8_t* out_partials) {
    return spectre_gpu_msm_g1_shard_device_timed(ctx, dev, d_bases, d_scalars,
                                                 n, flags, out_partials,
                                                 nullptr);
}

int spectre_gpu_msm_g1_shard_device_timed(spectre_gpu_ctx* ctx, int dev,
                                          const void* d_bases,
                                          const void* d_scalars, uint64_t n,
                                          uint32_t flags,
                                          uint8_t* out_partials,
                                          double out_ms[8]) {
    if (check_dev(ctx, dev)) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    return msm_device(ctx, dev, msm_call(d_bases, d_scalars, 1, n, flags),
                      (g1_jac*)out_partials, out_ms, /*sync=*/true, 0);
}

int spectre_gpu_msm_g1_shard_device_async(spectre_gpu_ctx* ctx, int dev,
                                          const void* d_bases,
                                          const void* d_scalars, uint64_t n,
                                          uint32_t flags,
                                          uint8_t* out_partials,
                                          int* out_slot) {
    return spectre_gpu_msm_g1_shard_windows_device_async(
        ctx, dev, d_bases, d_scalars, n, flags, 0, MSM_NWIN, out_partials,
        out_slot);
}

// window-sharded multi-GPU: rank r of R computes windows
// [r*NWIN/R, (r+1)*NWIN/R) over ALL n points. out_partials = w_cnt * 96 B.
int spectre_gpu_msm_g1_shard_windows_device(spectre_gpu_ctx* ctx, int dev,
                                            const void* d_bases,
                                            const void* d_scalars, uint64_t n,
                                            uint32_t flags, uint32_t w_lo,
                                            uint32_t w_cnt,
                                            uint8_t* out_partials) {
    if (check_dev(ctx, dev)) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    MsmCall call = msm_call(d_bases, d_scalars, 1, n, flags);
    call.w_lo = w_lo;
    call.w_cnt = w_cnt;
    return msm_device(ctx, dev, call, (g1_jac*)out_partials, nullptr,
                      /*sync=*/true, 0);
}

int spectre_gpu_msm_g1_shard_windows_device_async(
    spectre_gpu_ctx* ctx, int dev, const void* d_bases, const void* d_scalars,
    uint64_t n, uint32_t flags, uint32_t w_lo, uint32_t w_cnt,
    uint8_t* out_partials, int* out_slot) {
    if (check_dev(ctx, dev)) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    MsmCall call = msm_call(d_bases, d_scalars, 1, n, flags);
    call.w_lo = w_lo;
    call.w_cnt = w_cnt;
    *out_slot = next_async_slot(ctx->devs[dev]);
    return msm_device(ctx, dev, call, (g1_jac*)out_partials, nullptr,
                      /*sync=*/false, *out_slot);
}

// assemble disjoint per-shard window slices (shard i = NWIN/nshards
// consecutive windows, rank order) and finish with the window Horner.
int spectre_gpu_msm_g1_combine_windows(const uint8_t* partials,
                                       uint32_t nshards,
                                       uint8_t out_affine[64]) {
    if (!partials || nshards == 0 || MSM_NWIN % nshards != 0) {
        set_err("combine_windows: nshards must divide %d", MSM_NWIN);
        return -1;
    }
    winsums_to_affine((const g1_jac*)partials, out_affine);
    return 0;
}

int spectre_gpu_msm_slot_wait(spectre_gpu_ctx* ctx, int dev, int slot) {
    if (check_dev(ctx, dev)) return -1;
    if (slot < 0 || slot >= MSM_SLOTS) {
        set_err("slot_wait: slot %d out of range", slot);
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    return msm_slot_drain(ctx, dev, slot);
}

int spectre_gpu_msm_g1_device(spectre_gpu_ctx* ctx, int dev,
                              const void* d_bases, const void* d_scalars,
                              uint64_t n, uint32_t flags,
                              uint8_t out_affine[64]) {
    return spectre_gpu_msm_g1_batch_device(ctx, dev, d_bases, d_scalars, 1, n,
                                           flags, out_affine);
}

int spectre_gpu_msm_g1_batch_device(spectre_gpu_ctx* ctx, int dev,
                                    const void* d_bases,
                                    const void* d_scalars, uint32_t nbatch,
                                    uint64_t n, uint32_t flags,
                                    uint8_t* out_affine) {
    if (check_dev(ctx, dev)) return -1;
    if (check_nbatch(nbatch)) return -3;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    std::vector<g1_jac> wins((size_t)nbatch * MSM_NWIN);
    RC_TRY(msm_device(ctx, dev, msm_call(d_bases, d_scalars, nbatch, n, flags),
                      wins.data(), nullptr, /*sync=*/true, 0));
    for (uint32_t b = 0; b < nbatch; b++)
        winsums_to_affine(&wins[(size_t)b * MSM_NWIN], out_affine + 64 * b);
    return 0;
}

// scalars of a host-pointer call: plain scratch upload
static int upload_scalars(DeviceState& ds, const uint8_t* src, size_t bytes) {
    RC_TRY(ds.d_scalars.reserve(bytes));
    return staged_upload(ds, ds.d_scalars.ptr, src, bytes);
}

// Device pointer to the `count` bases at src: the cache entry of (bases_id,
// total_n, layout) when bases_id != 0 — uploaded on a miss, src may be NULL
// on a hit — else the uncached scratch buffer. A device's chunk of a
// sharded set depends on all three key words.
static int resolve_bases(DeviceState& ds, uint64_t bases_id, uint64_t layout,
                         uint64_t total_n, const uint8_t* src, uint64_t count,
                         const g1_affine** d_out) {
    const std::array<uint64_t, 3> key{bases_id, total_n, layout};
    DevBuf<g1_affine>* buf = &ds.d_bases;
    if (bases_id != 0) {
        auto it = ds.bases_cache.find(key);
        if (it != ds.bases_cache.end()) {
            *d_out = it->second.ptr;
            return 0;
        }
        if (!src) {
            set_err("bases_id %llu not cached and bases is NULL",
                    (unsigned long long)bases_id);
            return -4;
        }
        buf = &ds.bases_cache[key];
    } else if (!src) {
        set_err("bases is NULL");
        return -1;
    }
    int rc = buf->reserve(count);
    if (rc == 0) rc = staged_upload(ds, buf->ptr, src, count * 64);
    if (rc == 0) {
        *d_out = buf->ptr;
    } else if (bases_id != 0) {  // never cache a half-uploaded entry
        buf->release();
        ds.bases_cache.erase(key);
    }
    return rc;
}

int spectre_gpu_msm_g1_batch(spectre_gpu_ctx* ctx, uint64_t bases_id,
                             const uint8_t* bases, const uint8_t* scalars,
                             uint32_t nbatch, uint64_t n, uint32_t flags,
                             uint8_t* out_affine) {
    if (!ctx) {
        set_err("null ctx");
        return -1;
    }
    if (check_nbatch(nbatch)) return -3;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n == 0) {
        memset(out_affine, 0, (size_t)64 * nbatch);
        return 0;
    }
    if (!scalars) {
        set_err("scalars is NULL");
        return -1;
    }
    DeviceState& ds = ctx->devs[0];
    HIP_TRY(hipSetDevice(ds.device_id));
    RC_TRY(upload_scalars(ds, scalars, (size_t)nbatch * n * 32));
    const g1_affine* d_b = nullptr;
    RC_TRY(resolve_bases(ds, bases_id, 1, n, bases, n, &d_b));
    return spectre_gpu_msm_g1_batch_device(ctx, 0, d_b, ds.d_scalars.ptr,
                                           nbatch, n, flags, out_affine);
}

// upload + enqueue one device's shard of an n-point MSM split num_gpus ways
// (returns with async work in flight on that device's stream).
static int msm_multi_enqueue_one(spectre_gpu_ctx* ctx, int d, int num_gpus,
                                 uint64_t bases_id, const uint8_t* bases,
                                 const uint8_t* scalars, uint64_t n,
                                 uint32_t flags, g1_jac* wins_out) {
    DeviceState& ds = ctx->devs[d];
    HIP_TRY(hipSetDevice(ds.device_id));
    const uint64_t lo = n * d / num_gpus, hi = n * (d + 1) / num_gpus;
    const uint64_t m = hi - lo;
    RC_TRY(upload_scalars(ds, scalars + lo * 32, m * 32));
    const g1_affine* d_b = nullptr;
    RC_TRY(resolve_bases(ds, bases_id, (uint64_t)num_gpus, n,
                         bases ? bases + lo * 64 : nullptr, m, &d_b));
    // enqueue without synchronizing so all shards run concurrently
    return msm_device(ctx, d, msm_call(d_b, ds.d_scalars.ptr, 1, m, flags),
                      wins_out, nullptr, /*sync=*/false, 0);
}

int spectre_gpu_msm_g1(spectre_gpu_ctx* ctx, uint64_t bases_id,
                       const uint8_t* bases, const uint8_t* scalars, uint64_t n,
                       uint32_t flags, int num_gpus, uint8_t out_affine[64]) {
    if (!ctx) {
        set_err("null ctx");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n == 0) {
        memset(out_affine, 0, 64);
        return 0;
    }
    if (num_gpus <= 0) num_gpus = 1;
    if (num_gpus > (int)ctx->devs.size()) {
        set_err("num_gpus %d > ctx devices %zu", num_gpus, ctx->devs.size());
        return -1;
    }
    if (!scalars) {
        set_err("scalars is NULL");
        return -1;
    }
    std::vector<g1_jac> wins((size_t)num_gpus * MSM_NWIN);
    for (int d = 0; d < num_gpus; d++) {
        int rc = msm_multi_enqueue_one(ctx, d, num_gpus, bases_id, bases,
                                       scalars, n, flags,
                                       &wins[(size_t)d * MSM_NWIN]);
        if (rc) {
            // Devices <= d may have kernels and a pending hand-off into
            // `wins` in flight; drain them while the vector is alive. The
            // first error is the one reported.
            const std::string first = g_last_error;
            for (int e = 0; e <= d; e++) (void)msm_slot_drain(ctx, e, 0);
            g_last_error = first;
            return rc;
        }
    }
    for (int d = 0; d < num_gpus; d++) RC_TRY(msm_slot_drain(ctx, d, 0));
    return spectre_gpu_msm_g1_combine((const uint8_t*)wins.data(),
                                      (uint32_t)num_gpus, out_affine);
}

// ---------------------------------------------------------------- NTT
uint32_t spectre_gpu_ntt_split(uint32_t log_n, int force3, uint32_t k[3]) {
    if (log_n == 0 || log_n > 28 || !k) return 0;
    k[0] = k[1] = k[2] = 0;
    return ntt_split(log_n, force3 != 0, k);
}

int spectre_gpu_ntt_fr_device(spectre_gpu_ctx* ctx, int dev, void* d_data,
                              uint32_t log_n, const uint8_t omega[32],
                              int inverse, const uint8_t* coset_gen) {
    if (check_dev(ctx, dev)) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 om, g;
    ff_from_bytes(om, omega);
    if (coset_gen) ff_from_bytes(g, coset_gen);
    return ntt_device(ctx, dev, (fp256*)d_data, log_n, om, inverse,
                      coset_gen ? &g : nullptr);
}

int spectre_gpu_ntt_fr_extend_device(spectre_gpu_ctx* ctx, int dev,
                                     const void* d_coeffs, uint32_t log_n,
                                     uint32_t ext_bits, void* d_out,
                                     const uint8_t omega_ext[32],
                                     const uint8_t* coset_gen) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_coeffs || !d_out || !omega_ext) {
        set_err("ntt_extend: null %s",
                omega_ext ? "device pointer" : "omega_ext");
        return -1;
    }
    if (log_n > 28 || ext_bits > 28 - log_n) {
        set_err("ntt_extend: log_n %u + ext_bits %u > 28 unsupported (Fr "
                "2-adicity)", log_n, ext_bits);
        return -3;
    }
    // d_out is d_coeffs or lies clear of its n elements
    if (d_coeffs != d_out &&
        ranges_overlap(d_coeffs, 32ull << log_n, d_out,
                       32ull << (log_n + ext_bits))) {
        set_err("ntt_extend: d_out overlaps d_coeffs without being equal");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 om, g;
    ff_from_bytes(om, omega_ext);
    if (coset_gen) ff_from_bytes(g, coset_gen);
    return ntt_extend_device(ctx, dev, (const fp256*)d_coeffs, log_n, ext_bits,
                             (fp256*)d_out, om, coset_gen ? &g : nullptr);
}

int spectre_gpu_ntt_fr(spectre_gpu_ctx* ctx, uint8_t* data, uint32_t log_n,
                       const uint8_t omega[32], int inverse,
                       const uint8_t* coset_gen) {
    if (check_dev(ctx, 0)) return -1;
    if (log_n > 28) {
        set_err("ntt: log_n %u > 28 unsupported (Fr 2-adicity)", log_n);
        return -3;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    DeviceState& ds = ctx->devs[0];
    HIP_TRY(hipSetDevice(ds.device_id));
    const uint64_t n = 1ull << log_n;
    // cached IO buffer: the Rust seam calls this entry ~40-60x per proof and
    // must not pay a (up to 1 GB) hipMalloc/hipFree per transform.
    RC_TRY(ds.d_ntt_io.reserve(n));
    RC_TRY(staged_upload(ds, ds.d_ntt_io.ptr, data, n * 32));
    RC_TRY(spectre_gpu_ntt_fr_device(ctx, 0, ds.d_ntt_io.ptr, log_n, omega,
                                     inverse, coset_gen));
    return staged_download(ds, data, ds.d_ntt_io.ptr, n * 32);
}

int spectre_gpu_fr_gate_eval(spectre_gpu_ctx* ctx, int dev,
                             const void* const* d_cols, uint32_t ncols,
                             const uint8_t* constants, uint32_t nconst,
                             const uint32_t* program, uint32_t nops,
                             uint64_t n, uint32_t rot_scale, const uint8_t* y,
                             void* d_out) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_cols || !program || !nops || !d_out || (nconst && !constants)) {
        set_err("gate_eval: bad arguments");
        return -1;
    }
    // every column, read by the program or not, is a buffer clear of d_out:
    // with a rotation a lane reads rows that other lanes write
    for (uint32_t j = 0; j < ncols; j++) {
        if (!d_cols[j]) {
            set_err("gate_eval: null device pointer in d_cols[%u]", j);
            return -1;
        }
        if (ranges_overlap(d_cols[j], 32 * n, d_out, 32 * n)) {
            set_err("gate_eval: d_out overlaps d_cols[%u]", j);
            return -1;
        }
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 yv;
    if (y) ff_from_bytes(yv, y);
    return fr_gate_eval_device(ctx, dev, (const fp256* const*)d_cols, ncols,
                               (const fp256*)constants, nconst, program, nops,
                               n, rot_scale, y ? &yv : nullptr,
                               (fp256*)d_out);
}

int spectre_gpu_fr_vec_op(spectre_gpu_ctx* ctx, int dev, int op,
                          const void* d_a, const void* d_b, const uint8_t* c,
                          void* d_out, uint64_t n) {
    if (check_dev(ctx, dev)) return -1;
    if (op < 0 || op > 4 || !d_a || !d_out ||
        (op <= 2 && !d_b) || (op == 4 && !d_b) || (op >= 3 && !c)) {
        set_err("fr_vec_op: bad op/arguments");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 cv;
    if (c) ff_from_bytes(cv, c);
    return fr_vec_op_device(ctx, dev, op, (const fp256*)d_a,
                            (const fp256*)d_b, c ? &cv : nullptr,
                            (fp256*)d_out, n);
}

int spectre_gpu_fr_vec_mul_periodic(spectre_gpu_ctx* ctx, int dev,
                                    const void* d_a, const uint8_t* table,
                                    uint32_t period, void* d_out, uint64_t n) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_a || !d_out || !table) {
        set_err("fr_vec_mul_periodic: null %s",
                table ? "device pointer" : "table");
        return -1;
    }
    if (period == 0 || (period & (period - 1)) ||
        period > SPECTRE_VEC_PERIOD_MAX) {
        set_err("fr_vec_mul_periodic: period %u is not a power of two in "
                "[1, %u]", period, SPECTRE_VEC_PERIOD_MAX);
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 tab[SPECTRE_VEC_PERIOD_MAX];
    for (uint32_t j = 0; j < period; j++) ff_from_bytes(tab[j], table + 32 * j);
    return fr_vec_mul_periodic_device(ctx, dev, (const fp256*)d_a, tab, period,
                                      (fp256*)d_out, n);
}

// ---------------------------------------------------------------- grand products
int spectre_gpu_fr_batch_invert(spectre_gpu_ctx* ctx, int dev,
                                const void* d_in, void* d_out, uint64_t n) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_in || !d_out) {
        set_err("fr_batch_invert: null device pointer");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    return fr_batch_invert_device(ctx, dev, (const fp256*)d_in, (fp256*)d_out,
                                  n);
}

int spectre_gpu_fr_grand_product(spectre_gpu_ctx* ctx, int dev,
                                 const void* d_num, const void* d_den,
                                 const uint8_t z0[32], void* d_z, uint64_t n,
                                 uint8_t out_last[32]) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_num || !d_z) {
        set_err("fr_grand_product: null device pointer");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 last;
    RC_TRY(fr_grand_product_device(ctx, dev, (const fp256*)d_num,
                                   (const fp256*)d_den, fr_or_one(z0),
                                   (fp256*)d_z, n, out_last ? &last : nullptr));
    if (out_last) ff_to_bytes(out_last, last);
    return 0;
}

int spectre_gpu_set_fr_scan_tile(spectre_gpu_ctx* ctx, uint32_t elems) {
    if (!ctx || !fr_scan_tile_valid(elems)) {
        set_err("set_fr_scan_tile: %u is not 0 or a multiple of 256 <= %u",
                elems, fr_scan_tile_default());
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->fr_scan_tile = elems;
    return 0;
}

uint32_t spectre_gpu_fr_scan_tile_default(void) {
    return fr_scan_tile_default();
}

// ---------------------------------------------------------------- opening phase
int spectre_gpu_fr_poly_eval(spectre_gpu_ctx* ctx, int dev,
                             const void* d_coeffs, uint64_t n,
                             const uint8_t* points, uint32_t npoints,
                             uint8_t* out) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_coeffs || !points || !out) {
        set_err("fr_poly_eval: null %s",
                d_coeffs ? "points/out" : "device pointer");
        return -1;
    }
    if (npoints < 1 || npoints > SPECTRE_POLY_EVAL_MAX_POINTS) {
        set_err("fr_poly_eval: npoints %u outside [1, %u]", npoints,
                SPECTRE_POLY_EVAL_MAX_POINTS);
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 pts[SPECTRE_POLY_EVAL_MAX_POINTS], vals[SPECTRE_POLY_EVAL_MAX_POINTS];
    for (uint32_t p = 0; p < npoints; p++) ff_from_bytes(pts[p], points + 32 * p);
    RC_TRY(fr_poly_eval_device(ctx, dev, (const fp256*)d_coeffs, n, pts,
                               npoints, vals));
    for (uint32_t p = 0; p < npoints; p++) ff_to_bytes(out + 32 * p, vals[p]);
    return 0;
}

int spectre_gpu_fr_poly_div_linear(spectre_gpu_ctx* ctx, int dev,
                                   const void* d_a, const uint8_t z[32],
                                   void* d_q, uint64_t n,
                                   uint8_t out_rem[32]) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_a || !d_q || !z) {
        set_err("fr_poly_div_linear: null %s",
                z ? "device pointer" : "z");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 zv, rem;
    ff_from_bytes(zv, z);
    RC_TRY(fr_poly_div_linear_device(ctx, dev, (const fp256*)d_a, zv,
                                     (fp256*)d_q, n, out_rem ? &rem : nullptr));
    if (out_rem) ff_to_bytes(out_rem, rem);
    return 0;
}

// a host array of m device pointers, 1 <= m <= SPECTRE_OPEN_MAX_POLYS, none
// of them null
static int check_poly_list(const char* what, const void* const* d_polys,
                           uint32_t m) {
    if (m < 1 || m > SPECTRE_OPEN_MAX_POLYS) {
        set_err("%s: m %u outside [1, %u]", what, m, SPECTRE_OPEN_MAX_POLYS);
        return -1;
    }
    if (!d_polys) {
        set_err("%s: null pointer array", what);
        return -1;
    }
    for (uint32_t k = 0; k < m; k++) {
        if (!d_polys[k]) {
            set_err("%s: null device pointer d_polys[%u]", what, k);
            return -1;
        }
    }
    return 0;
}

int spectre_gpu_fr_lincomb(spectre_gpu_ctx* ctx, int dev,
                           const void* const* d_polys, const uint8_t* coeffs,
                           uint32_t m, void* d_out, uint64_t n) {
    if (check_dev(ctx, dev)) return -1;
    RC_TRY(check_poly_list("fr_lincomb", d_polys, m));
    if (!coeffs) {
        set_err("fr_lincomb: null coeffs");
        return -1;
    }
    if (n > (1ull << 28)) {
        set_err("fr_lincomb: n %llu > 2^28", (unsigned long long)n);
        return -1;
    }
    if (n == 0) return 0;
    if (!d_out) {
        set_err("fr_lincomb: null device pointer d_out");
        return -1;
    }
    // d_out is an input or lies clear of its n elements
    for (uint32_t k = 0; k < m; k++) {
        if (d_polys[k] != d_out &&
            ranges_overlap(d_polys[k], 32 * n, d_out, 32 * n)) {
            set_err("fr_lincomb: d_out overlaps d_polys[%u] without being "
                    "equal", k);
            return -1;
        }
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 cv[SPECTRE_OPEN_MAX_POLYS];
    for (uint32_t k = 0; k < m; k++) ff_from_bytes(cv[k], coeffs + 32 * k);
    return fr_lincomb_device(ctx, dev, (const fp256* const*)d_polys, cv, m,
                             (fp256*)d_out, n);
}

int spectre_gpu_fr_poly_eval_batch(spectre_gpu_ctx* ctx, int dev,
                                   const void* const* d_polys, uint32_t m,
                                   uint64_t n, const uint8_t* points,
                                   uint32_t npoints, uint8_t* out) {
    if (check_dev(ctx, dev)) return -1;
    RC_TRY(check_poly_list("fr_poly_eval_batch", d_polys, m));
    if (!points || !out) {
        set_err("fr_poly_eval_batch: null points/out");
        return -1;
    }
    if (npoints < 1 || npoints > SPECTRE_POLY_EVAL_MAX_POINTS) {
        set_err("fr_poly_eval_batch: npoints %u outside [1, %u]", npoints,
                SPECTRE_POLY_EVAL_MAX_POINTS);
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 pts[SPECTRE_POLY_EVAL_MAX_POINTS];
    std::vector<fp256> vals((size_t)m * npoints);
    for (uint32_t p = 0; p < npoints; p++) ff_from_bytes(pts[p], points + 32 * p);
    RC_TRY(fr_poly_eval_batch_device(ctx, dev, (const fp256* const*)d_polys, m,
                                     n, pts, npoints, vals.data()));
    for (size_t v = 0; v < vals.size(); v++) ff_to_bytes(out + 32 * v, vals[v]);
    return 0;
}

int spectre_gpu_fr_poly_div_roots(spectre_gpu_ctx* ctx, int dev,
                                  const void* d_a, const uint8_t* roots,
                                  uint32_t nroots, void* d_q, uint64_t n,
                                  uint8_t* out_rems) {
    if (check_dev(ctx, dev)) return -1;
    if (!d_a || !d_q || !roots) {
        set_err("fr_poly_div_roots: null %s",
                roots ? "device pointer" : "roots");
        return -1;
    }
    if (nroots < 1 || nroots > SPECTRE_POLY_EVAL_MAX_POINTS) {
        set_err("fr_poly_div_roots: nroots %u outside [1, %u]", nroots,
                SPECTRE_POLY_EVAL_MAX_POINTS);
        return -1;
    }
    if (n > (1ull << 28)) {
        set_err("fr_poly_div_roots: n %llu > 2^28", (unsigned long long)n);
        return -1;
    }
    if (d_a != d_q && ranges_overlap(d_a, 32 * n, d_q, 32 * n)) {
        set_err("fr_poly_div_roots: d_q overlaps d_a without being equal");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 zs[SPECTRE_POLY_EVAL_MAX_POINTS], rems[SPECTRE_POLY_EVAL_MAX_POINTS];
    for (uint32_t j = 0; j < nroots; j++) ff_from_bytes(zs[j], roots + 32 * j);
    RC_TRY(fr_poly_div_roots_device(ctx, dev, (const fp256*)d_a, zs, nroots,
                                    (fp256*)d_q, n,
                                    out_rems ? rems : nullptr));
    for (uint32_t j = 0; out_rems && j < nroots; j++)
        ff_to_bytes(out_rems + 32 * j, rems[j]);
    return 0;
}

// ---------------------------------------------------------------- lookup argument
int spectre_gpu_fr_lookup_permute(spectre_gpu_ctx* ctx, int dev,
                                  const void* d_input, const void* d_table,
                                  void* d_input_perm, void* d_table_perm,
                                  uint64_t u) {
    if (check_dev(ctx, dev)) return -1;
    const void* buf[4] = {d_input, d_table, d_input_perm, d_table_perm};
    static const char* const name[4] = {"d_input", "d_table", "d_input_perm",
                                        "d_table_perm"};
    for (int i = 0; i < 4; i++) {
        if (!buf[i]) {
            set_err("fr_lookup_permute: null device pointer %s", name[i]);
            return -1;
        }
    }
    if (u > (1ull << 28)) {
        set_err("fr_lookup_permute: u %llu > 2^28", (unsigned long long)u);
        return -1;
    }
    for (int i = 0; i < 4; i++) {
        for (int j = i + 1; j < 4; j++) {
            if (ranges_overlap(buf[i], 32 * u, buf[j], 32 * u)) {
                set_err("fr_lookup_permute: %s and %s overlap", name[i],
                        name[j]);
                return -1;
            }
        }
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    return fr_lookup_permute_device(ctx, dev, (const fp256*)d_input,
                                    (const fp256*)d_table,
                                    (fp256*)d_input_perm,
                                    (fp256*)d_table_perm, u);
}

// ---------------------------------------------------------------- permutation argument
int spectre_gpu_fr_powers(spectre_gpu_ctx* ctx, int dev, const uint8_t c[32],
                          const uint8_t g[32], void* d_out, uint64_t n) {
    if (check_dev(ctx, dev)) return -1;
    if (!g) {
        set_err("fr_powers: null g");
        return -3;
    }
    if (n > (1ull << 28)) {
        set_err("fr_powers: n %llu > 2^28", (unsigned long long)n);
        return -3;
    }
    if (n == 0) return 0;
    if (!d_out) {
        set_err("fr_powers: null device pointer d_out");
        return -3;
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 gv;
    ff_from_bytes(gv, g);
    return fr_powers_device(ctx, dev, fr_or_one(c), gv, (fp256*)d_out, n);
}

int spectre_gpu_fr_permutation_terms(
    spectre_gpu_ctx* ctx, int dev, const void* const* d_values,
    const void* const* d_sigmas, uint32_t m, const uint8_t beta[32],
    const uint8_t gamma[32], const uint8_t omega[32], const uint8_t delta0[32],
    const uint8_t delta[32], void* d_num, void* d_den, uint64_t n) {
    if (check_dev(ctx, dev)) return -1;
    if (m < 1 || m > SPECTRE_PERM_MAX_COLS) {
        set_err("fr_permutation_terms: m %u outside [1, %u]", m,
                SPECTRE_PERM_MAX_COLS);
        return -3;
    }
    if (n > (1ull << 28)) {
        set_err("fr_permutation_terms: n %llu > 2^28", (unsigned long long)n);
        return -3;
    }
    if (!d_values || !d_sigmas || !beta || !gamma || !omega || !delta) {
        set_err("fr_permutation_terms: null %s",
                d_values && d_sigmas ? "beta/gamma/omega/delta"
                                     : "column pointer array");
        return -3;
    }
    if (n == 0) return 0;
    if (!d_num || !d_den) {
        set_err("fr_permutation_terms: null device pointer %s",
                d_num ? "d_den" : "d_num");
        return -3;
    }
    // the outputs lie clear of each other and of every input
    const void* const out[2] = {d_num, d_den};
    if (ranges_overlap(d_num, 32 * n, d_den, 32 * n)) {
        set_err("fr_permutation_terms: d_num and d_den overlap");
        return -3;
    }
    for (uint32_t j = 0; j < m; j++) {
        const void* const in[2] = {d_values[j], d_sigmas[j]};
        for (int k = 0; k < 2; k++) {
            if (!in[k]) {
                set_err("fr_permutation_terms: null device pointer %s[%u]",
                        k ? "d_sigmas" : "d_values", j);
                return -3;
            }
            for (int o = 0; o < 2; o++) {
                if (ranges_overlap(in[k], 32 * n, out[o], 32 * n)) {
                    set_err("fr_permutation_terms: %s overlaps %s[%u]",
                            o ? "d_den" : "d_num",
                            k ? "d_sigmas" : "d_values", j);
                    return -3;
                }
            }
        }
    }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    fp256 b, g, w, d;
    ff_from_bytes(b, beta);
    ff_from_bytes(g, gamma);
    ff_from_bytes(w, omega);
    ff_from_bytes(d, delta);
    return fr_permutation_terms_device(
        ctx, dev, (const fp256* const*)d_values, (const fp256* const*)d_sigmas,
        m, b, g, w, fr_or_one(delta0), d, (fp256*)d_num, (fp256*)d_den, n);
}

// ---------------------------------------------------------------- memory
int spectre_gpu_malloc(spectre_gpu_ctx* ctx, int dev, size_t bytes,
                       void** d_ptr) {
    if (check_dev(ctx, dev)) return -1;
    HIP_TRY(hipSetDevice(ctx->devs[dev].device_id));
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return 0;
}
int spectre_gpu_free(spectre_gpu_ctx* ctx, int dev, void* d_ptr) {
    if (check_dev(ctx, dev)) return -1;
    HIP_TRY(hipSetDevice(ctx->devs[dev].device_id));
    HIP_TRY(hipFree(d_ptr));
    return 0;
}
int spectre_gpu_upload(spectre_gpu_ctx* ctx, int dev, void* d_dst,
                       const void* src, size_t bytes) {
    if (check_dev(ctx, dev)) return -1;
    HIP_TRY(hipSetDevice(ctx->devs[dev].device_id));
    HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
int spectre_gpu_download(spectre_gpu_ctx* ctx, int dev, void* dst,
                         const void* d_src, size_t bytes) {
    if (check_dev(ctx, dev)) return -1;
    HIP_TRY(hipSetDevice(ctx->devs[dev].device_id));
    HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int spectre_gpu_synchronize(spectre_gpu_ctx* ctx, int dev) {
    if (check_dev(ctx, dev)) return -1;
    HIP_TRY(hipSetDevice(ctx->devs[dev].device_id));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

}  // extern "C"
