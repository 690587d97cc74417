// extern "C" surface of libdca_hip.so (see include/dca_hip.h).
#include <cstdlib>

#include "dca_internal.h"
#include "align_plan.h"
#include "assignment.h"

static thread_local char g_err[1024] = "";

void dca_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

void dca_flush_clocks(dca_ctx* ctx)
{
    for (auto& kv : ctx->clocks) {
        for (auto& pr : kv.second.pending) {
            float ms = 0.f;
            hipEventSynchronize(pr.second);
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) kv.second.ms += ms;
            hipEventDestroy(pr.first);
            hipEventDestroy(pr.second);
        }
        kv.second.pending.clear();
    }
}

// ---- device block cache (declared in dca_internal.h)
#include <mutex>
#include <unordered_map>
namespace {
struct DevBlock { void* p; size_t bytes; int device; };
struct DevPool {
    std::mutex mu;
    std::unordered_map<void*, DevBlock> live;     // blocks handed out that are eligible for caching
    std::vector<DevBlock> cached;
    size_t cachedBytes = 0;
    size_t maxBytes = getenv("DCA_POOL_MAX_BYTES") ? strtoull(getenv("DCA_POOL_MAX_BYTES"), nullptr, 10) : ((size_t)64 << 30);
    void release_all() {          // caller holds mu
        for (auto& b : cached) { hipSetDevice(b.device); hipFree(b.p); }
        cached.clear(); cachedBytes = 0;
    }
};
DevPool& pool() { static DevPool* p = new DevPool(); return *p; }   // never destroyed: the HIP runtime may be gone at exit
constexpr size_t kPoolMinBytes = (size_t)1 << 20;
std::atomic<size_t> g_blocksInUse{0};      // handed out by dca_dev_malloc, not yet given to dca_dev_free (dca_device_blocks_in_use)
hipError_t pool_malloc(void** out, size_t bytes, bool zero_recycled);
}  // namespace

hipError_t dca_dev_malloc(void** out, size_t bytes, bool zero_recycled)
{
    *out = nullptr;
    const hipError_t e = bytes < kPoolMinBytes ? hipMalloc(out, bytes) : pool_malloc(out, bytes, zero_recycled);
    if (e == hipSuccess) g_blocksInUse.fetch_add(1, std::memory_order_relaxed);
    return e;
}

namespace {
hipError_t pool_malloc(void** out, size_t bytes, bool zero_recycled)
{
    int dev = 0;
    hipGetDevice(&dev);
    DevPool& P = pool();
    void* hit = nullptr;
    size_t hitBytes = 0;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        int best = -1;
        for (int i = 0; i < (int)P.cached.size(); ++i) {
            const DevBlock& b = P.cached[i];
            if (b.device != dev || b.bytes < bytes || b.bytes > bytes + bytes / 4) continue;
            if (best < 0 || b.bytes < P.cached[best].bytes) best = i;
        }
        if (best >= 0) {
            hit = P.cached[best].p; hitBytes = P.cached[best].bytes;
            P.cachedBytes -= hitBytes;
            P.cached.erase(P.cached.begin() + best);
            P.live[hit] = DevBlock{hit, hitBytes, dev};
        }
    }
    if (hit) {
        // a fresh hipMalloc block reads as zeros; keep that for recycled ones (the copy engine fills > 3 TB/s)
        if (zero_recycled) {
            hipError_t e = hipMemsetAsync(hit, 0, bytes, nullptr);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) return e;
        }
        *out = hit;
        return hipSuccess;
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) {        // out of memory: give the cache back and try once more
        (void)hipGetLastError();
        { std::lock_guard<std::mutex> lk(P.mu); P.release_all(); }
        e = hipMalloc(out, bytes);
        if (e != hipSuccess) return e;
    }
    std::lock_guard<std::mutex> lk(P.mu);
    P.live[*out] = DevBlock{*out, bytes, dev};
    return hipSuccess;
}
}  // namespace

hipError_t dca_dev_free(void* p)
{
    if (!p) return hipSuccess;
    g_blocksInUse.fetch_sub(1, std::memory_order_relaxed);
    DevPool& P = pool();
    DevBlock b{nullptr, 0, 0};
    {
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.live.find(p);
        if (it != P.live.end()) { b = it->second; P.live.erase(it); }
    }
    if (!b.p) return hipFree(p);
    // same guarantee as hipFree: nothing on the device still uses the block when this returns
    int cur = 0;
    hipGetDevice(&cur);
    if (cur != b.device) hipSetDevice(b.device);
    hipError_t e = hipDeviceSynchronize();
    if (cur != b.device) hipSetDevice(cur);
    std::lock_guard<std::mutex> lk(P.mu);
    if (e != hipSuccess || P.cachedBytes + b.bytes > P.maxBytes) {
        hipSetDevice(b.device); hipError_t f = hipFree(b.p); hipSetDevice(cur);
        return f;
    }
    P.cached.push_back(b);
    P.cachedBytes += b.bytes;
    return hipSuccess;
}

#define CHECK_CTX(ctx)                                             \
    do {                                                           \
        if (!(ctx)) { dca_set_error("null context"); return DCA_ERR_ARG; } \
        hipError_t _e = hipSetDevice((ctx)->device);               \
        if (_e != hipSuccess) { dca_set_error("hipSetDevice: %s", hipGetErrorString(_e)); return DCA_ERR_HIP; } \
    } while (0)

namespace {
// dst[n][0..Ls) = src[n][0..L), zero padded; *maxCode = the largest code met (the range check of dca_set_msa, on the device: a
// pass over the 25 MB of config D costs the host 2.5 ms)
__global__ void pad_rows_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int N, int L, int Ls, unsigned* __restrict__ maxCode)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    unsigned v = 0;
    if (t < (size_t)N * Ls) {
        const size_t n = t / Ls;
        const int c = (int)(t % Ls);
        v = c < L ? src[n * L + c] : 0u;
        dst[t] = (uint8_t)v;
    }
    // wave maximum, one atomic per wave that holds a code above the smallest alphabet
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off));
    // (read first: after the first few waves nobody has anything larger to report -- 800 000 atomics on one word cost config E 8 ms)
    if ((threadIdx.x & 63) == 0 && v > __hip_atomic_load(maxCode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxCode, v);
}
__global__ void unpad_rows_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int N, int L, int Ls)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)N * L) return;
    dst[t] = src[(t / L) * Ls + t % L];
}
}  // namespace

extern "C" {

const char* dca_last_error(void) { return g_err; }
const char* dca_version(void) { return "pydca_amd libdca_hip 0.1 (gfx950)"; }

size_t dca_release_cached_memory(void)
{
    DevPool& P = pool();
    std::lock_guard<std::mutex> lk(P.mu);
    const size_t n = P.cachedBytes;
    int cur = 0;
    hipGetDevice(&cur);
    P.release_all();
    hipSetDevice(cur);
    return n;
}

size_t dca_device_blocks_in_use(void) { return g_blocksInUse.load(std::memory_order_relaxed); }

int dca_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t dca_plm_num_params(int L, int q)
{
    return (size_t)L * q + (size_t)L * (L - 1) / 2 * (size_t)q * q;
}

int dca_read_msa(const char* path, int biomolecule, int L, uint8_t* out, int capacity, int* raw_count)
{
    return dca_read_msa_impl(path, biomolecule, L, out, capacity, raw_count);
}

int dca_count_msa_lines(const char* path) { return dca_count_msa_lines_impl(path); }
int dca_encode_sequences(const char* seqs, const int* offsets, int nseq, int biomolecule, int table, int L, uint8_t* out, int* bad_record)
{
    return dca_encode_sequences_impl(seqs, offsets, nseq, biomolecule, table, L, out, bad_record);
}
int dca_read_msa_alloc(const char* path, int biomolecule, int L, uint8_t** rows, int* raw_count)
{
    if (!rows) { dca_set_error("dca_read_msa_alloc: bad arguments"); return DCA_ERR_ARG; }
    return dca_read_msa_owned(path, biomolecule, L, rows, raw_count);
}

int dca_create(dca_ctx** out, int device, int precision)
{
    if (!out || (precision != DCA_F32 && precision != DCA_F64)) { dca_set_error("dca_create: bad arguments"); return DCA_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        dca_set_error("no HIP device visible: libdca_hip has no CPU fallback");
        return DCA_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { dca_set_error("device %d out of range (%d visible)", device, ndev); return DCA_ERR_ARG; }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        dca_set_error("device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return DCA_ERR_NO_DEVICE;
    }
    dca_ctx* ctx = new dca_ctx();
    ctx->device = device;
    ctx->precision = precision;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = dca_dev_alloc(&ctx->dScal, 64);
    if (e == hipSuccess) e = hipHostMalloc(&ctx->hScal, 64 * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {                       // nothing half-built is handed out or left behind
        dca_set_error("dca_create: %s", hipGetErrorString(e));
        dca_destroy(ctx);
        return DCA_ERR_HIP;
    }
    *out = ctx;
    return DCA_OK;
}

static void free_msa(dca_ctx* ctx)
{
    dca_bm_free(ctx);
    delete ctx->plm; ctx->plm = nullptr;
    dca_free_ar_engine(ctx->ar); ctx->ar = nullptr;
    if (ctx->mf) { dca_free_mf_engine(ctx->mf); ctx->mf = nullptr; }
    dca_dev_free(ctx->dX); ctx->dX = nullptr;
    dca_dev_free(ctx->dCounts); ctx->dCounts = nullptr;
    dca_dev_free(ctx->dWd); ctx->dWd = nullptr;
    dca_dev_free(ctx->dLastScores); ctx->dLastScores = nullptr; ctx->nLastScores = 0;
    ctx->hX.clear();
    ctx->have_weights = ctx->have_counts = false;
}

}  // extern "C" (internal C++ helpers follow)

const uint8_t* dca_host_msa(dca_ctx* ctx)
{
    if (ctx->hX.empty() && ctx->dX) {
        ctx->hX.resize((size_t)ctx->N * ctx->L);
        DevBuf<uint8_t> dTmp;
        hipError_t e = dTmp.alloc(ctx->hX.size());
        if (e == hipSuccess) {
            hipLaunchKernelGGL(unpad_rows_kernel, dim3((unsigned)((ctx->hX.size() + 255) / 256)), dim3(256), 0, ctx->stream,
                               ctx->dX, dTmp.get(), ctx->N, ctx->L, ctx->Ls);
            e = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess) e = hipMemcpy(ctx->hX.data(), dTmp, ctx->hX.size(), hipMemcpyDeviceToHost);
        }
        if (e != hipSuccess) {
            ctx->hX.clear();
            dca_set_error("copying the alignment back to the host failed: %s", hipGetErrorString(e));
            return nullptr;
        }
    }
    return ctx->hX.empty() ? nullptr : ctx->hX.data();
}

int dca_remember_scores(dca_ctx* ctx, const double* dScores, int n)
{
    if (ctx->nLastScores != n) {
        dca_dev_free(ctx->dLastScores); ctx->dLastScores = nullptr; ctx->nLastScores = 0;
        HIP_TRY(dca_dev_alloc(&ctx->dLastScores, (size_t)n));
        ctx->nLastScores = n;
    }
    HIP_TRY(hipMemcpyAsync(ctx->dLastScores, dScores, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return DCA_OK;
}

extern "C" {

void dca_destroy(dca_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    dca_comm_destroy_impl(ctx);
    dca_flush_clocks(ctx);
    free_msa(ctx);
    dca_dev_free(ctx->dScal);
    if (ctx->hScal) hipHostFree(ctx->hScal);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int dca_set_msa(dca_ctx* ctx, const uint8_t* X, int N, int L, int q)
{
    CHECK_CTX(ctx);
    // (one site is enough for the distance entries; the models ask for two themselves)
    if (!X || N <= 0 || L < 1 || q < 2 || q > 32) { dca_set_error("dca_set_msa: bad arguments"); return DCA_ERR_ARG; }
    free_msa(ctx);
    ctx->N = ctx->L = ctx->q = ctx->Ls = 0;                // the context holds no alignment until everything below succeeded
    const int Ls = (int)round_up((size_t)L, 128);
    ctx->hX.clear();                                       // host copy is made on demand (dca_host_msa)
    // one contiguous copy + a repack kernel (a pitched hipMemcpy2D of narrow rows takes seconds)
    DevBuf<uint8_t> dTmp;
    DevBuf<unsigned> dMax;
    unsigned maxCode = 0;
    hipError_t e = dca_dev_alloc(&ctx->dX, (size_t)N * Ls);
    if (e == hipSuccess) e = dTmp.alloc((size_t)N * L);
    if (e == hipSuccess) e = dMax.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(dMax, 0, sizeof(unsigned), ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(dTmp, X, (size_t)N * L, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const size_t total = (size_t)N * Ls;
        hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, dTmp.get(), ctx->dX, N, L, Ls, dMax.get());
        e = hipMemcpyAsync(&maxCode, dMax, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    dTmp.reset();
    dMax.reset();
    if (e == hipSuccess && maxCode >= (unsigned)q) {      // the slow search only runs on failure
        size_t k = 0;
        while (X[k] < q) ++k;
        free_msa(ctx);
        dca_set_error("dca_set_msa: code %d >= q at element %zu", (int)X[k], k);
        return DCA_ERR_ARG;
    }
    if (e == hipSuccess) e = dca_dev_alloc(&ctx->dCounts, (size_t)N);
    if (e == hipSuccess) e = dca_dev_alloc(&ctx->dWd, (size_t)N);
    if (e != hipSuccess) {
        free_msa(ctx);
        dca_set_error("uploading the alignment: %s", hipGetErrorString(e));
        return DCA_ERR_HIP;
    }
    ctx->N = N; ctx->L = L; ctx->q = q; ctx->Ls = Ls;
    return DCA_OK;
}

// Everything the engines derived from the weights (the plmDCA engine's copy, frequencies, counts, correlation matrix,
// couplings) is dropped when the weights change: the next call recomputes it instead of answering for the old weights.
// The engines themselves stay (with their reduce / comm hooks, native-comm mode and vector sharding): a sharded context that
// is re-weighted must not fall back to unreduced local sums.  The plmDCA engine has to be configured again.
static void weights_changed(dca_ctx* ctx)
{
    dca_bm_free(ctx);          // a Boltzmann-learning run fits the old weights' statistics: it ends
    if (ctx->plm) ctx->plm->weights_changed();
    dca_ar_engine_weights_changed(ctx->ar);       // the autoregressive engine keeps x and must be configured again
    if (ctx->mf) dca_mf_engine_invalidate(ctx->mf);
}

int dca_compute_weights(dca_ctx* ctx, double seqid, int compare_precision)
{
    CHECK_CTX(ctx);
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (compare_precision != DCA_F32 && compare_precision != DCA_F64) return DCA_ERR_ARG;
    weights_changed(ctx);
    return dca_weights_compute(ctx, seqid, compare_precision);
}

int dca_weights_partial_counts(dca_ctx* ctx, double seqid, int compare_precision, int part, int parts, uint32_t* counts_out)
{
    CHECK_CTX(ctx);
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (compare_precision != DCA_F32 && compare_precision != DCA_F64) return DCA_ERR_ARG;
    weights_changed(ctx);
    DCA_TRY(dca_weights_compute(ctx, seqid, compare_precision, part, parts, false));
    if (counts_out) HIP_TRY(hipMemcpy(counts_out, ctx->dCounts, (size_t)ctx->N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCA_OK;
}

int dca_set_weight_counts(dca_ctx* ctx, const uint32_t* counts)
{
    CHECK_CTX(ctx);
    if (!ctx->dX || !counts) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    for (int n = 0; n < ctx->N; ++n)
        if (counts[n] == 0) { dca_set_error("dca_set_weight_counts: count of sequence %d is zero (every sequence counts itself)", n); return DCA_ERR_ARG; }
    weights_changed(ctx);
    HIP_TRY(hipMemcpy(ctx->dCounts, counts, (size_t)ctx->N * sizeof(uint32_t), hipMemcpyHostToDevice));
    return dca_weights_finish(ctx);
}

int dca_compute_weights_sharded(dca_ctx* ctx, double seqid, int compare_precision)
{
    CHECK_CTX(ctx);
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (compare_precision != DCA_F32 && compare_precision != DCA_F64) return DCA_ERR_ARG;
    if (!ctx->comm) { dca_set_error("no communicator: dca_comm_init first"); return DCA_ERR_STATE; }
    weights_changed(ctx);
    DCA_TRY(dca_weights_compute(ctx, seqid, compare_precision, ctx->comm_rank, ctx->comm_world, false));
    DCA_TRY(dca_comm_native_sum_u32(ctx, ctx->dCounts, (size_t)ctx->N));       // integer sums: exact, order-free
    return dca_weights_finish(ctx);
}

int dca_set_weights(dca_ctx* ctx, const double* w)
{
    CHECK_CTX(ctx);
    if (!ctx->dX || !w) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    weights_changed(ctx);
    HIP_TRY(hipMemcpy(ctx->dWd, w, (size_t)ctx->N * sizeof(double), hipMemcpyHostToDevice));
    double s = 0;
    for (int n = 0; n < ctx->N; ++n) s += w[n];
    ctx->meff = s;
    ctx->have_weights = true;
    ctx->have_counts = false;
    return DCA_OK;
}

int dca_get_weights(dca_ctx* ctx, double* w_out)
{
    CHECK_CTX(ctx);
    if (!ctx->have_weights) { dca_set_error("weights not available"); return DCA_ERR_STATE; }
    HIP_TRY(hipMemcpy(w_out, ctx->dWd, (size_t)ctx->N * sizeof(double), hipMemcpyDeviceToHost));
    return DCA_OK;
}

int dca_weights_work(dca_ctx* ctx, uint64_t* out3)
{
    if (!ctx || !out3) return DCA_ERR_ARG;
    out3[0] = ctx->weightsWork[0]; out3[1] = ctx->weightsWork[1]; out3[2] = (uint64_t)ctx->weightsPlanes;
    return DCA_OK;
}

int dca_get_weight_counts(dca_ctx* ctx, uint32_t* counts_out)
{
    CHECK_CTX(ctx);
    if (!ctx->have_counts) { dca_set_error("counts not available"); return DCA_ERR_STATE; }
    HIP_TRY(hipMemcpy(counts_out, ctx->dCounts, (size_t)ctx->N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCA_OK;
}

int dca_get_meff(dca_ctx* ctx, double* meff_out)
{
    if (!ctx || !ctx->have_weights) { dca_set_error("weights not available"); return DCA_ERR_STATE; }
    *meff_out = ctx->meff;
    return DCA_OK;
}

// ------------------------------------------------------------------ plmDCA
static int need_plm(dca_ctx* ctx)
{
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (ctx->L < 2) { dca_set_error("the model needs an alignment of at least two sites"); return DCA_ERR_STATE; }
    if (!ctx->plm) ctx->plm = dca_make_plm_engine(ctx);
    return DCA_OK;
}

int dca_plm_configure(dca_ctx* ctx, double lambda_h, double lambda_J, int carry_mode, int chunk, int warmup, int halo, int add_regulariser)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (carry_mode < 0 || carry_mode > 2) return DCA_ERR_ARG;
    dca_bm_free(ctx);
    return ctx->plm->configure(lambda_h, lambda_J, carry_mode, chunk, warmup, halo, add_regulariser);
}
int dca_plm_configure_strips(dca_ctx* ctx, double lambda_h, double lambda_J, int carry_mode, int chunk, int warmup)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (carry_mode < 0 || carry_mode > 2) return DCA_ERR_ARG;
    dca_bm_free(ctx);
    return ctx->plm->configure_strips(lambda_h, lambda_J, carry_mode, chunk, warmup);
}
int dca_plm_release(dca_ctx* ctx)
{
    CHECK_CTX(ctx);
    if (!ctx->plm) return DCA_OK;
    // the engine's kernels may still be running on the context's stream
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { dca_set_error("dca_plm_release: stream synchronisation failed"); return DCA_ERR_HIP; }
    dca_bm_free(ctx);
    delete ctx->plm; ctx->plm = nullptr;
    return DCA_OK;
}
int dca_plm_init_x(dca_ctx* ctx) { CHECK_CTX(ctx); DCA_TRY(need_plm(ctx)); return ctx->plm->init_x(); }
int dca_plm_set_x(dca_ctx* ctx, const void* x, int dtype) { CHECK_CTX(ctx); DCA_TRY(need_plm(ctx)); return ctx->plm->set_x(x, dtype); }
int dca_plm_get_x(dca_ctx* ctx, void* x, int dtype) { CHECK_CTX(ctx); DCA_TRY(need_plm(ctx)); return ctx->plm->get_x(x, dtype); }
int dca_plm_get_g(dca_ctx* ctx, void* g, int dtype) { CHECK_CTX(ctx); DCA_TRY(need_plm(ctx)); return ctx->plm->get_g(g, dtype); }
int dca_plm_gradient(dca_ctx* ctx, double* fx_out) { CHECK_CTX(ctx); DCA_TRY(need_plm(ctx)); return ctx->plm->gradient(fx_out); }
int dca_plm_set_vector_sharding(dca_ctx* ctx, int rank, int world, dca_comm_hook hook, void* user)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    return ctx->plm->set_vector_sharding(rank, world, hook, user);
}
int dca_plm_set_reduce_hook(dca_ctx* ctx, dca_reduce_hook hook, void* user)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (hook && ctx->plm->native_mode == 4) { dca_set_error("configured for column strips: no reduce hook"); return DCA_ERR_STATE; }
    ctx->plm->hook = hook;
    ctx->plm->hook_user = user;
    if (hook && ctx->plm->native_mode == 1) ctx->plm->native_mode = 0;      // the hook replaces the native all-reduce
    return DCA_OK;
}
int dca_plm_lbfgs_begin(dca_ctx* ctx, int max_iterations, int verbose)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    dca_bm_free(ctx);
    return ctx->plm->lbfgs_begin(max_iterations, verbose);
}
int dca_plm_lbfgs_iterate(dca_ctx* ctx, int iterations, dca_plm_stats* st) { CHECK_CTX(ctx); DCA_TRY(need_plm(ctx)); return ctx->plm->lbfgs_iterate(iterations, st); }
int dca_plm_lbfgs_end(dca_ctx* ctx) { CHECK_CTX(ctx); if (ctx->plm) ctx->plm->lbfgs_end(); return DCA_OK; }
int dca_plm_scores(dca_ctx* ctx, int apc, double* out) { CHECK_CTX(ctx); DCA_TRY(need_plm(ctx)); return ctx->plm->scores(apc, out); }
int dca_plm_energies(dca_ctx* ctx, const uint8_t* X, int n, double* energies_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (n < 0 || (n > 0 && (!X || !energies_out))) return DCA_ERR_ARG;
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, false));
    return dca_potts_energies(ctx, ps, X, n, energies_out);
}
int dca_plm_mutation_scan(dca_ctx* ctx, const uint8_t* wildtype, double* dE_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (!wildtype || !dE_out) return DCA_ERR_ARG;
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, false));
    return dca_potts_mutation_scan(ctx, ps, wildtype, dE_out);
}
int dca_plm_pseudo_likelihood(dca_ctx* ctx, const uint8_t* X, int n, double* pll_out, double* site_out, double* cond_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (n < 0 || (n > 0 && (!X || !pll_out))) return DCA_ERR_ARG;
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, false));
    return dca_potts_pseudo_likelihood(ctx, ps, X, n, pll_out, site_out, cond_out);
}
int dca_plm_sample(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep, double beta,
                   const uint8_t* initial, uint8_t* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, false));
    return dca_potts_sample(ctx, ps, n, sweeps, seed, first_chain, first_sweep, beta, initial, out);
}
// conditional Gibbs sampling (sample_conditional.hip) of the plm engine's x; one GPU only
int dca_plm_sample_conditional(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep, double beta,
                               const int32_t* free_sites, int num_free, const uint8_t* initial, int random_start, uint8_t* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, true));
    return dca_potts_sample_conditional(ctx, ps, n, sweeps, seed, first_chain, first_sweep, beta, free_sites, num_free, initial,
                                        random_start, out);
}
// inter-protein energies (interaction.hip) under the plm engine's x; one GPU only
int dca_plm_interaction_energies(dca_ctx* ctx, int split, const uint8_t* XA, int nA, const uint8_t* XB, int nB, const int32_t* offsets_a,
                                 const int32_t* offsets_b, int G, int gauge, double* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, true));
    return dca_potts_interaction_energies(ctx, ps, split, XA, nA, XB, nB, offsets_a, offsets_b, G, gauge, out);
}
// greedy ascent to local maxima (ascent.hip) under the plm engine's x; one GPU only
int dca_plm_ascend(dca_ctx* ctx, const uint8_t* X, int n, const int32_t* free_sites, int num_free, int max_steps, double min_gain,
                   uint8_t* out, int32_t* steps_out, uint8_t* converged_out, double* gain_out, int32_t* path_out, double* path_gain_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, true));
    return dca_potts_ascend(ctx, ps, X, n, free_sites, num_free, max_steps, min_gain, out, steps_out, converged_out, gain_out, path_out,
                            path_gain_out);
}
// replica-exchange Gibbs sampling (tempered.hip) under the plm engine's x; one GPU only
int dca_plm_sample_tempered(dca_ctx* ctx, const dca_pt_args* args, uint8_t* out, int32_t* levels_out, double* energies_out,
                            uint64_t* attempts_out, uint64_t* accepts_out, double* energy_trace_out, int* rounds_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, true));
    return dca_potts_sample_tempered(ctx, ps, args, out, levels_out, energies_out, attempts_out, accepts_out, energy_trace_out, rounds_out);
}
// annealed importance sampling (ais.hip) of the plm engine's x
int dca_plm_ais(dca_ctx* ctx, const dca_ais_args* args, double* log_weights_out, double* log_z0_out, uint8_t* chains_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (!args || !log_weights_out) { dca_set_error("dca_plm_ais: args or log_weights_out is NULL"); return DCA_ERR_ARG; }
    PottsSource ps;
    DCA_TRY(ctx->plm->potts_source(&ps, true));
    return dca_potts_ais(ctx, ps, args, log_weights_out, log_z0_out, chains_out);
}
// Boltzmann learning (boltzmann.hip) on the plm engine's x
int dca_plm_bm_begin(dca_ctx* ctx, const dca_bm_args* args)
{
    CHECK_CTX(ctx);
    if (!args) { dca_set_error("dca_plm_bm_begin: args is NULL"); return DCA_ERR_ARG; }
    DCA_TRY(need_plm(ctx));
    void* dx = nullptr;
    DCA_TRY(ctx->plm->bm_source(&dx));
    return dca_bm_begin_impl(ctx, dx, ctx->precision == DCA_F64 ? DCA_F64 : DCA_F32, args);
}
int dca_plm_bm_iterate(dca_ctx* ctx, int iterations, dca_bm_record* records_out)
{
    CHECK_CTX(ctx);
    if (!ctx->bm || !ctx->plm) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    void* dx = nullptr;
    DCA_TRY(ctx->plm->bm_source(&dx));
    return dca_bm_iterate_impl(ctx, dx, iterations, records_out);
}
int dca_plm_bm_freqs(dca_ctx* ctx, int which, double* fi_out, double* fij_out) { CHECK_CTX(ctx); return dca_bm_freqs_impl(ctx, which, fi_out, fij_out); }
int dca_plm_bm_chains(dca_ctx* ctx, uint8_t* out) { CHECK_CTX(ctx); return dca_bm_chains_impl(ctx, out); }
int dca_plm_bm_end(dca_ctx* ctx) { CHECK_CTX(ctx); dca_bm_free(ctx); return DCA_OK; }
// the mask, the decimation and the gauge (decimation.hip)
int dca_plm_bm_set_mask(dca_ctx* ctx, const uint8_t* mask)
{
    CHECK_CTX(ctx);
    if (!ctx->bm || !ctx->plm) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    void* dx = nullptr;
    DCA_TRY(ctx->plm->bm_source(&dx));
    return dca_bm_set_mask_impl(ctx, dx, mask);
}
int dca_plm_bm_get_mask(dca_ctx* ctx, uint8_t* out) { CHECK_CTX(ctx); return dca_bm_get_mask_impl(ctx, out); }
int dca_plm_bm_decimate(dca_ctx* ctx, long long remove, double* scores_out, dca_bm_decimation* info)
{
    CHECK_CTX(ctx);
    if (!ctx->bm || !ctx->plm) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    void* dx = nullptr;
    DCA_TRY(ctx->plm->bm_source(&dx));
    return dca_bm_decimate_impl(ctx, dx, remove, scores_out, info);
}
int dca_plm_zero_sum_gauge(dca_ctx* ctx)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (dca_bm_has_removed(ctx)) {
        dca_set_error("dca_plm_zero_sum_gauge: the Boltzmann run's mask has removed elements, which the transformation would fill again");
        return DCA_ERR_STATE;
    }
    void* dx = nullptr;
    DCA_TRY(ctx->plm->transform_source(&dx));
    return dca_zero_sum_gauge_impl(ctx, dx, ctx->precision == DCA_F64 ? DCA_F64 : DCA_F32);
}

// ------------------------------------------------------------------ sequence sets against the alignment (distance.hip, set_stats.hip)
int dca_hamming_nearest(dca_ctx* ctx, const uint8_t* Q, int nq, const uint8_t* R, int nr, int skip_same_index,
                        int32_t* dist_out, int32_t* index_out, uint64_t* hist_out)
{
    CHECK_CTX(ctx);
    if (!dist_out) { dca_set_error("dca_hamming_nearest: dist_out is NULL"); return DCA_ERR_ARG; }
    if (!ctx->dX) { dca_set_error("dca_hamming_nearest: dca_set_msa first (the alignment gives L and q, and is the reference set when R is NULL)"); return DCA_ERR_STATE; }
    if ((Q && nq < 1) || (R && nr < 1)) { dca_set_error("dca_hamming_nearest: nq %d, nr %d must be >= 1", nq, nr); return DCA_ERR_ARG; }
    return dca_hamming_nearest_impl(ctx, Q, nq, R, nr, skip_same_index != 0, dist_out, index_out, hist_out);
}
int dca_sequence_statistics(dca_ctx* ctx, const uint8_t* Q, int nq, double* fi_out, double* fij_out, dca_set_comparison* cmp_out)
{
    CHECK_CTX(ctx);
    if (!Q || nq < 1) { dca_set_error("dca_sequence_statistics: Q is NULL or nq %d < 1", nq); return DCA_ERR_ARG; }
    if (!fi_out && !fij_out && !cmp_out) { dca_set_error("dca_sequence_statistics: every output is NULL"); return DCA_ERR_ARG; }
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (ctx->L < 2) { dca_set_error("dca_sequence_statistics: the alignment needs at least two sites"); return DCA_ERR_STATE; }
    if (cmp_out && !ctx->have_weights) { dca_set_error("dca_sequence_statistics: dca_compute_weights or dca_set_weights first"); return DCA_ERR_STATE; }
    return dca_set_statistics_impl(ctx, Q, nq, fi_out, fij_out, cmp_out);
}
int dca_alignment_statistics(dca_ctx* ctx, double* fi_out, double* fij_out)
{
    CHECK_CTX(ctx);
    if (!fi_out && !fij_out) { dca_set_error("dca_alignment_statistics: both outputs are NULL"); return DCA_ERR_ARG; }
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (ctx->L < 2) { dca_set_error("dca_alignment_statistics: the alignment needs at least two sites"); return DCA_ERR_STATE; }
    if (!ctx->have_weights) { dca_set_error("dca_alignment_statistics: dca_compute_weights or dca_set_weights first"); return DCA_ERR_STATE; }
    return dca_set_statistics_impl(ctx, nullptr, 0, fi_out, fij_out, nullptr);
}

// ------------------------------------------------------------------ profile alignment (align.hip)
int dca_profile_align(dca_ctx* ctx, const int32_t* match, int Lp, int A, const int32_t* del_open, const int32_t* del_extend,
                      int ins_open, int ins_extend, int mode, const uint8_t* seqs, const int64_t* offsets, int n,
                      int32_t* score_out, int32_t* residue_at_out)
{
    static const char* who = "dca_profile_align";
    CHECK_CTX(ctx);
    if (!match || !del_open || !del_extend || !offsets || !score_out || (!seqs && n > 0 && offsets[n] > offsets[0])) {
        dca_set_error("%s: a required pointer is NULL", who);
        return DCA_ERR_ARG;
    }
    if (Lp < 1 || Lp > kAlignMaxLp) { dca_set_error("%s: Lp %d is outside 1 .. %d", who, Lp, kAlignMaxLp); return DCA_ERR_ARG; }
    if (A < 2 || A > kAlignMaxA) { dca_set_error("%s: A %d is outside 2 .. %d", who, A, kAlignMaxA); return DCA_ERR_ARG; }
    if (mode != DCA_ALIGN_LOCAL && mode != DCA_ALIGN_GLOCAL) { dca_set_error("%s: mode %d is neither DCA_ALIGN_LOCAL nor DCA_ALIGN_GLOCAL", who, mode); return DCA_ERR_ARG; }
    if (n < 0) { dca_set_error("%s: n %d < 0", who, n); return DCA_ERR_ARG; }
    long long maxMatch = 0, maxPenalty = std::max(std::llabs((long long)ins_open), std::llabs((long long)ins_extend));
    if (ins_open > 0 || ins_extend > 0) { dca_set_error("%s: ins_open %d and ins_extend %d must be <= 0", who, ins_open, ins_extend); return DCA_ERR_ARG; }
    for (int i = 0; i < Lp; ++i) {
        if (del_open[i] > 0 || del_extend[i] > 0) {
            dca_set_error("%s: del_open %d / del_extend %d of column %d must be <= 0", who, del_open[i], del_extend[i], i);
            return DCA_ERR_ARG;
        }
        maxPenalty = std::max(maxPenalty, std::max(std::llabs((long long)del_open[i]), std::llabs((long long)del_extend[i])));
    }
    for (size_t k = 0; k < (size_t)Lp * A; ++k) maxMatch = std::max(maxMatch, std::llabs((long long)match[k]));
    if (!align_values_in_range(maxMatch, maxPenalty, Lp)) {
        dca_set_error("%s: (max|match| %lld + max|penalty| %lld) * (Lp + 32767) reaches 2^28: the sums could overflow", who, maxMatch, maxPenalty);
        return DCA_ERR_ARG;
    }
    for (int k = 0; k < n; ++k) {
        const long long len = offsets[k + 1] - offsets[k];
        if (len < 0 || len > kAlignMaxLen) { dca_set_error("%s: record %d has %lld residues (0 .. %d)", who, k, len, kAlignMaxLen); return DCA_ERR_ARG; }
        for (long long j = offsets[k]; j < offsets[k + 1]; ++j)
            if (seqs[j] >= A) { dca_set_error("%s: code %d >= A at residue %lld of record %d", who, (int)seqs[j], j - offsets[k], k); return DCA_ERR_ARG; }
    }
    return dca_profile_align_impl(ctx, match, Lp, A, del_open, del_extend, ins_open, ins_extend, mode, seqs, offsets, n, score_out,
                                  residue_at_out, &ctx->alignScratchBytes);
}
int dca_get_msa(dca_ctx* ctx, uint8_t* out)
{
    CHECK_CTX(ctx);
    if (!out) { dca_set_error("dca_get_msa: out is NULL"); return DCA_ERR_ARG; }
    if (!ctx->dX) { dca_set_error("dca_get_msa: dca_set_msa first"); return DCA_ERR_STATE; }
    const uint8_t* X = dca_host_msa(ctx);
    if (!X) return DCA_ERR_HIP;
    memcpy(out, X, (size_t)ctx->N * ctx->L);
    return DCA_OK;
}
int dca_profile_align_last_scratch(dca_ctx* ctx, unsigned long long* bytes_out)
{
    CHECK_CTX(ctx);
    if (!bytes_out) { dca_set_error("dca_profile_align_last_scratch: bytes_out is NULL"); return DCA_ERR_ARG; }
    *bytes_out = ctx->alignScratchBytes;
    return DCA_OK;
}
int dca_sw_scores_device(dca_ctx* ctx, const char* ref, int lref, const char* seqs, const int* offsets, int nseq, const int* sub,
                         int gap_open, int gap_extend, int* scores_out)
{
    CHECK_CTX(ctx);
    if (!ref || !seqs || !offsets || !sub || !scores_out || nseq < 0) { dca_set_error("dca_sw_scores_device: bad arguments"); return DCA_ERR_ARG; }
    if (lref < 1 || lref > kAlignMaxLp) { dca_set_error("dca_sw_scores_device: lref %d is outside 1 .. %d", lref, kAlignMaxLp); return DCA_ERR_ARG; }
    // the query profile: 26 letters plus "other", which scores -4 against everything as sub_score (host_io.cpp) does
    constexpr int A = 27;
    const int Lp = lref;
    std::vector<int32_t> match((size_t)Lp * A, -4), open((size_t)Lp, gap_open), extend((size_t)Lp, gap_extend);
    for (int i = 0; i < Lp; ++i) {
        const int ia = (unsigned char)ref[i] - 'A';
        if (ia < 0 || ia >= 26) continue;
        for (int b = 0; b < 26; ++b) match[(size_t)i * A + b] = sub[ia * 26 + b];
    }
    std::vector<int64_t> offs((size_t)nseq + 1);
    for (int k = 0; k <= nseq; ++k) offs[k] = offsets[k] - offsets[0];
    std::vector<uint8_t> codes((size_t)std::max<int64_t>(offs[nseq], 1));
    for (int64_t j = 0; j < offs[nseq]; ++j) {
        const int ib = (unsigned char)seqs[offsets[0] + j] - 'A';
        codes[j] = (uint8_t)(ib < 0 || ib >= 26 ? 26 : ib);
    }
    static_assert(sizeof(int) == sizeof(int32_t), "scores_out is filled as int32");
    return dca_profile_align(ctx, match.data(), Lp, A, open.data(), extend.data(), gap_open, gap_extend, DCA_ALIGN_LOCAL, codes.data(),
                             offs.data(), nseq, reinterpret_cast<int32_t*>(scores_out), nullptr);
}

// ------------------------------------------------------------------ redundancy filter and identity clusters (redundancy.hip)
static int identity_arguments(dca_ctx* ctx, const char* who, const uint8_t* X, int n, int min_identical)
{
    if (!ctx->dX) { dca_set_error("%s: dca_set_msa first (the alignment gives L and q, and is the row set when X is NULL)", who); return DCA_ERR_STATE; }
    if (X && n < 1) { dca_set_error("%s: n %d must be >= 1", who, n); return DCA_ERR_ARG; }
    if (min_identical < 1 || min_identical > ctx->L + 1) {
        dca_set_error("%s: min_identical %d is outside 1 .. L + 1 = %d", who, min_identical, ctx->L + 1);
        return DCA_ERR_ARG;
    }
    return DCA_OK;
}
int dca_identity_filter(dca_ctx* ctx, const uint8_t* X, int n, int min_identical, const int32_t* order, uint8_t* keep_out,
                        int32_t* rep_out, dca_filter_info* info)
{
    CHECK_CTX(ctx);
    if (!keep_out) { dca_set_error("dca_identity_filter: keep_out is NULL"); return DCA_ERR_ARG; }
    DCA_TRY(identity_arguments(ctx, "dca_identity_filter", X, n, min_identical));
    return dca_identity_filter_impl(ctx, X, n, min_identical, order, keep_out, rep_out, info);
}
int dca_identity_clusters(dca_ctx* ctx, const uint8_t* X, int n, int min_identical, int32_t* label_out, int32_t* degree_out,
                          dca_cluster_info* info)
{
    CHECK_CTX(ctx);
    if (!label_out) { dca_set_error("dca_identity_clusters: label_out is NULL"); return DCA_ERR_ARG; }
    DCA_TRY(identity_arguments(ctx, "dca_identity_clusters", X, n, min_identical));
    return dca_identity_clusters_impl(ctx, X, n, min_identical, label_out, degree_out, info);
}

static int three_site_state(dca_ctx* ctx, const char* who, const uint8_t* Q, int nq)
{
    if (!ctx->dX) { dca_set_error("%s: dca_set_msa first", who); return DCA_ERR_STATE; }
    if (ctx->L < 3) { dca_set_error("%s: three-site correlations need an alignment of at least three sites, not %d", who, ctx->L); return DCA_ERR_ARG; }
    if (Q && nq < 1) { dca_set_error("%s: nq %d < 1", who, nq); return DCA_ERR_ARG; }
    if (!Q && !ctx->have_weights) { dca_set_error("%s: dca_compute_weights or dca_set_weights first (Q is NULL: the alignment under its weights)", who); return DCA_ERR_STATE; }
    return DCA_OK;
}
int dca_three_site_values(dca_ctx* ctx, const uint8_t* Q, int nq, const int32_t* elements, int T, uint64_t* count_out,
                          uint64_t* denom_out, double* f3_out, double* c3_out)
{
    CHECK_CTX(ctx);
    if (!elements || T < 1) { dca_set_error("dca_three_site_values: elements is NULL or T %d < 1", T); return DCA_ERR_ARG; }
    if (!count_out && !denom_out && !f3_out && !c3_out) { dca_set_error("dca_three_site_values: every output is NULL"); return DCA_ERR_ARG; }
    DCA_TRY(three_site_state(ctx, "dca_three_site_values", Q, nq));
    return dca_three_site_values_impl(ctx, Q, nq, elements, T, count_out, denom_out, f3_out, c3_out);
}
int dca_three_site_scan(dca_ctx* ctx, const uint8_t* Q, int nq, int K, int skip_state, int32_t* elements_out, double* c3_out,
                        double* f3_out, int* found)
{
    CHECK_CTX(ctx);
    if (K < 1) { dca_set_error("dca_three_site_scan: K %d < 1", K); return DCA_ERR_ARG; }
    if (!elements_out || !found) { dca_set_error("dca_three_site_scan: elements_out or found is NULL"); return DCA_ERR_ARG; }
    DCA_TRY(three_site_state(ctx, "dca_three_site_scan", Q, nq));
    if (skip_state < -1 || skip_state >= ctx->q) { dca_set_error("dca_three_site_scan: skip_state %d is neither -1 nor a state < %d", skip_state, ctx->q); return DCA_ERR_ARG; }
    return dca_three_site_scan_impl(ctx, Q, nq, K, skip_state, elements_out, c3_out, f3_out, found);
}

int dca_pca_fit(dca_ctx* ctx, int k, double tol, int max_iterations, uint64_t seed, double* eigenvalues_out, double* components_out,
                double* offsets_out, double* residuals_out, double* total_variance_out, int* iterations_out, int* converged_out)
{
    CHECK_CTX(ctx);
    if (!eigenvalues_out || !components_out || !offsets_out || !converged_out) { dca_set_error("dca_pca_fit: eigenvalues_out, components_out, offsets_out or converged_out is NULL"); return DCA_ERR_ARG; }
    if (!(tol > 0.0)) { dca_set_error("dca_pca_fit: tol %g must be > 0", tol); return DCA_ERR_ARG; }
    if (max_iterations < 1) { dca_set_error("dca_pca_fit: max_iterations %d < 1", max_iterations); return DCA_ERR_ARG; }
    if (k < 1) { dca_set_error("dca_pca_fit: k %d < 1", k); return DCA_ERR_ARG; }
    if (!ctx->dX) { dca_set_error("dca_pca_fit: dca_set_msa first"); return DCA_ERR_STATE; }
    if (k > 64 || k > ctx->L * ctx->q) { dca_set_error("dca_pca_fit: k %d is more than min(64, L q = %d)", k, ctx->L * ctx->q); return DCA_ERR_ARG; }
    if (!ctx->have_weights) { dca_set_error("dca_pca_fit: dca_compute_weights or dca_set_weights first"); return DCA_ERR_STATE; }
    return dca_pca_fit_impl(ctx, k, tol, max_iterations, seed, eigenvalues_out, components_out, offsets_out, residuals_out,
                            total_variance_out, iterations_out, converged_out);
}
int dca_pca_project(dca_ctx* ctx, const uint8_t* Q, int nq, int k, const double* components, const double* offsets, double* proj_out)
{
    CHECK_CTX(ctx);
    if (!components || !offsets || !proj_out) { dca_set_error("dca_pca_project: components, offsets or proj_out is NULL"); return DCA_ERR_ARG; }
    if (k < 1) { dca_set_error("dca_pca_project: k %d < 1", k); return DCA_ERR_ARG; }
    if (Q && nq < 1) { dca_set_error("dca_pca_project: nq %d < 1", nq); return DCA_ERR_ARG; }
    if (!ctx->dX) { dca_set_error("dca_pca_project: dca_set_msa first"); return DCA_ERR_STATE; }
    return dca_pca_project_impl(ctx, Q, nq, k, components, offsets, proj_out);
}

int dca_plm_di_scores(dca_ctx* ctx, const double* reg_fi, int apc, double* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (!reg_fi || !out) return DCA_ERR_ARG;
    return ctx->plm->di_scores(reg_fi, apc, out);
}

// ------------------------------------------------------------------ mfDCA
static int need_mf(dca_ctx* ctx)
{
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (ctx->L < 2) { dca_set_error("the model needs an alignment of at least two sites"); return DCA_ERR_STATE; }
    if (!ctx->have_weights) { dca_set_error("weights must be computed or set first"); return DCA_ERR_STATE; }
    if (!ctx->mf) ctx->mf = dca_make_mf_engine(ctx);
    return ctx->mf ? DCA_OK : DCA_ERR_NOMEM;
}
// the mean-field model for the dca_potts_* calls; its device fields live until the call's stream work has drained
struct MfPotts {
    PottsSource ps{};
    DevBuf<double> dH;
    int get(dca_ctx* c) { return dca_mf_engine_potts_source(c->mf, &ps, &dH); }
};
int dca_mf_single_site_freqs(dca_ctx* ctx, double* fi_out) { CHECK_CTX(ctx); DCA_TRY(need_mf(ctx)); return dca_mf_engine_site_freqs(ctx->mf, fi_out); }
int dca_mf_pair_site_freqs(dca_ctx* ctx, double* fij_out) { CHECK_CTX(ctx); DCA_TRY(need_mf(ctx)); return dca_mf_engine_pair_freqs(ctx->mf, fij_out); }
int dca_mf_corr_mat(dca_ctx* ctx, double pseudocount, double* corr_out) { CHECK_CTX(ctx); DCA_TRY(need_mf(ctx)); return dca_mf_engine_corr(ctx->mf, pseudocount, corr_out); }
int dca_mf_couplings(dca_ctx* ctx, double* out) { CHECK_CTX(ctx); DCA_TRY(need_mf(ctx)); return dca_mf_engine_couplings(ctx->mf, out); }
int dca_mf_scores(dca_ctx* ctx, int apc, double* out) { CHECK_CTX(ctx); DCA_TRY(need_mf(ctx)); return dca_mf_engine_scores(ctx->mf, apc, out); }
int dca_plm_pair_couplings(dca_ctx* ctx, const int* pairs, int npairs, int shift, double* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_plm(ctx));
    if (npairs < 0 || (npairs > 0 && (!pairs || !out))) return DCA_ERR_ARG;
    return ctx->plm->pair_couplings(pairs, npairs, shift, out);
}
int dca_di_from_arrays(dca_ctx* ctx, const double* couplings, int layout, const double* reg_fi, int L, int q,
                       double* fields_out, double* di_out)
{
    CHECK_CTX(ctx);
    if (!couplings || !reg_fi || (layout != 1 && layout != 2) || (!fields_out && !di_out)) return DCA_ERR_ARG;
    return dca_di_from_arrays_impl(ctx, couplings, layout, reg_fi, L, q, fields_out, di_out);
}
int dca_di_from_fields(dca_ctx* ctx, const double* couplings, int layout, const double* reg_fi, const double* fields_ij,
                       int L, int q, double* di_out)
{
    CHECK_CTX(ctx);
    if (!couplings || !reg_fi || !fields_ij || !di_out || (layout != 1 && layout != 2)) return DCA_ERR_ARG;
    return dca_di_from_arrays_impl(ctx, couplings, layout, reg_fi, L, q, nullptr, di_out, fields_ij);
}
int dca_comm_unique_id(const char* rccl_path, void* id128)
{
    if (!id128) return DCA_ERR_ARG;
    return dca_comm_unique_id_impl(rccl_path, id128);
}
int dca_comm_init(dca_ctx* ctx, const char* rccl_path, const void* id128, int world, int rank)
{
    CHECK_CTX(ctx);
    if (!id128) return DCA_ERR_ARG;
    // slices and reductions configured for the previous communicator's world / rank do not carry over
    // (an engine in the middle of an optimisation refuses: its vector slices are cut for the old world, so the
    // communicator must not change under it -- DCA_ERR_STATE, nothing touched)
    if (ctx->comm) {
        if (ctx->plm && ctx->plm->configured_for_comm()) DCA_TRY(ctx->plm->set_native_comm(0));
        if (ctx->mf) dca_mf_engine_set_native(ctx->mf, false);
    }
    return dca_comm_init_impl(ctx, rccl_path, id128, world, rank);
}
int dca_comm_destroy(dca_ctx* ctx)
{
    CHECK_CTX(ctx);
    // giving the communicator back ends whatever optimisation was being driven over it (a caller that stops calling
    // dca_plm_lbfgs_iterate below its cap never reaches `finished`; without this the communicator could not be released)
    if (ctx->comm && ctx->plm) ctx->plm->lbfgs_end();
    if (ctx->comm && ctx->plm && ctx->plm->configured_for_comm()) DCA_TRY(ctx->plm->set_native_comm(0));
    if (ctx->mf) dca_mf_engine_set_native(ctx->mf, false);
    dca_comm_destroy_impl(ctx);
    return DCA_OK;
}
int dca_comm_abort(dca_ctx* ctx)
{
    if (!ctx) return DCA_ERR_ARG;          // no device switch, no stream work: this runs beside the thread that drives the context
    return dca_comm_abort_impl(ctx);
}
int dca_comm_info(dca_ctx* ctx, int* world, int* rank)
{
    CHECK_CTX(ctx);
    return dca_comm_info_impl(ctx, world, rank);
}
int dca_plm_set_native_comm(dca_ctx* ctx, int mode)
{
    CHECK_CTX(ctx);
    if (!ctx->plm) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
    return ctx->plm->set_native_comm(mode);        // drops the caller's hook only once the mode has been validated
}
int dca_mf_set_native_comm(dca_ctx* ctx, int on)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    if (on && !ctx->comm) { dca_set_error("no communicator: dca_comm_init first"); return DCA_ERR_STATE; }
    dca_mf_engine_set_native(ctx->mf, on != 0);
    return DCA_OK;
}
int dca_mf_set_row_window(dca_ctx* ctx, int first, int count)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    return dca_mf_engine_set_row_window(ctx->mf, first, count);
}
int dca_comm_allgather_host(dca_ctx* ctx, const double* mine, int n, double* all)
{
    CHECK_CTX(ctx);
    if (!mine || !all || n <= 0) return DCA_ERR_ARG;
    if (!ctx->comm) { dca_set_error("no communicator: dca_comm_init first"); return DCA_ERR_STATE; }
    const size_t total = (size_t)n * ctx->comm_world;
    DevBuf<double> d;
    HIP_TRY(d.alloc(total));
    // every rank contributes its values at its own offset of a zero vector: the sum IS the gathered vector (only sums are bound)
    if (hipMemsetAsync(d, 0, total * sizeof(double), ctx->stream) != hipSuccess ||
        hipMemcpyAsync(d + (size_t)n * ctx->comm_rank, mine, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return DCA_ERR_HIP;
    DCA_TRY(dca_comm_native(ctx, DCA_COMM_ALL_REDUCE, d, total, DCA_F64));
    if (hipMemcpyAsync(all, d, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) return DCA_ERR_HIP;
    return DCA_OK;
}
int dca_mf_set_reduce_hook(dca_ctx* ctx, dca_reduce_hook hook, void* user)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    dca_mf_engine_set_hook(ctx->mf, hook, user);
    return DCA_OK;
}
int dca_mf_fields(dca_ctx* ctx, double* out) { CHECK_CTX(ctx); DCA_TRY(need_mf(ctx)); if (!out) return DCA_ERR_ARG; return dca_mf_engine_fields(ctx->mf, out); }
int dca_mf_energies(dca_ctx* ctx, const uint8_t* X, int n, double* energies_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    if (n < 0 || (n > 0 && (!X || !energies_out))) return DCA_ERR_ARG;
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_energies(ctx, m.ps, X, n, energies_out);
}
int dca_mf_mutation_scan(dca_ctx* ctx, const uint8_t* wildtype, double* dE_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    if (!wildtype || !dE_out) return DCA_ERR_ARG;
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_mutation_scan(ctx, m.ps, wildtype, dE_out);
}
int dca_mf_pseudo_likelihood(dca_ctx* ctx, const uint8_t* X, int n, double* pll_out, double* site_out, double* cond_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    if (n < 0 || (n > 0 && (!X || !pll_out))) return DCA_ERR_ARG;
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_pseudo_likelihood(ctx, m.ps, X, n, pll_out, site_out, cond_out);
}
int dca_mf_sample(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep, double beta,
                  const uint8_t* initial, uint8_t* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_sample(ctx, m.ps, n, sweeps, seed, first_chain, first_sweep, beta, initial, out);
}
int dca_mf_sample_conditional(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep, double beta,
                              const int32_t* free_sites, int num_free, const uint8_t* initial, int random_start, uint8_t* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_sample_conditional(ctx, m.ps, n, sweeps, seed, first_chain, first_sweep, beta, free_sites, num_free, initial,
                                        random_start, out);
}
int dca_mf_interaction_energies(dca_ctx* ctx, int split, const uint8_t* XA, int nA, const uint8_t* XB, int nB, const int32_t* offsets_a,
                                const int32_t* offsets_b, int G, int gauge, double* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_interaction_energies(ctx, m.ps, split, XA, nA, XB, nB, offsets_a, offsets_b, G, gauge, out);
}
int dca_assign_partners(const double* E, int nr, int nc, int32_t* col_of_row, double* total_out, double* gap_out)
{
    if (assign_partners_host(E, nr, nc, col_of_row, total_out, gap_out) != 0) {
        dca_set_error("assign_partners: a negative size, a NULL array or a non-finite entry");
        return DCA_ERR_ARG;
    }
    return DCA_OK;
}
int dca_mf_ascend(dca_ctx* ctx, const uint8_t* X, int n, const int32_t* free_sites, int num_free, int max_steps, double min_gain,
                  uint8_t* out, int32_t* steps_out, uint8_t* converged_out, double* gain_out, int32_t* path_out, double* path_gain_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_ascend(ctx, m.ps, X, n, free_sites, num_free, max_steps, min_gain, out, steps_out, converged_out, gain_out, path_out,
                            path_gain_out);
}
int dca_mf_sample_tempered(dca_ctx* ctx, const dca_pt_args* args, uint8_t* out, int32_t* levels_out, double* energies_out,
                           uint64_t* attempts_out, uint64_t* accepts_out, double* energy_trace_out, int* rounds_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_sample_tempered(ctx, m.ps, args, out, levels_out, energies_out, attempts_out, accepts_out, energy_trace_out, rounds_out);
}
int dca_mf_ais(dca_ctx* ctx, const dca_ais_args* args, double* log_weights_out, double* log_z0_out, uint8_t* chains_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    if (!args || !log_weights_out) { dca_set_error("dca_mf_ais: args or log_weights_out is NULL"); return DCA_ERR_ARG; }
    MfPotts m;
    DCA_TRY(m.get(ctx));
    return dca_potts_ais(ctx, m.ps, args, log_weights_out, log_z0_out, chains_out);
}
int dca_mf_pair_couplings(dca_ctx* ctx, const int* pairs, int npairs, int shift, double* out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    if (npairs < 0 || (npairs > 0 && (!pairs || !out))) return DCA_ERR_ARG;
    return dca_mf_engine_pair_couplings(ctx->mf, pairs, npairs, shift, out);
}
int dca_scores_order(dca_ctx* ctx, int32_t* order_out, int capacity)
{
    CHECK_CTX(ctx);
    if (!ctx->dLastScores) { dca_set_error("no score vector has been computed on this context"); return DCA_ERR_STATE; }
    if (!order_out || capacity < ctx->nLastScores) return DCA_ERR_ARG;
    return dca_scores_order_device(ctx, ctx->dLastScores, ctx->nLastScores, order_out);
}
int dca_mf_di_scores(dca_ctx* ctx, int apc, double* out) { CHECK_CTX(ctx); DCA_TRY(need_mf(ctx)); return dca_mf_engine_di(ctx->mf, apc, out); }
int dca_mf_run(dca_ctx* ctx, double pseudocount, int apc, double* scores_out, double* couplings_out)
{
    CHECK_CTX(ctx);
    DCA_TRY(need_mf(ctx));
    DCA_TRY(dca_mf_engine_corr(ctx->mf, pseudocount, nullptr));
    DCA_TRY(dca_mf_engine_couplings(ctx->mf, couplings_out));
    return dca_mf_engine_scores(ctx->mf, apc, scores_out);
}

// ------------------------------------------------------------------ Hopfield-Potts
int dca_mf_hopfield_fit(dca_ctx* ctx, double pseudocount, const dca_hopfield_args* args, double* eigenvalues_out, double* gains_out,
                        int32_t* signs_out, double* patterns_out, double* residuals_out, dca_hopfield_info* info_out)
{
    static const char* who = "dca_mf_hopfield_fit";
    CHECK_CTX(ctx);
    if (!args || !eigenvalues_out || !gains_out || !signs_out || !patterns_out || !residuals_out || !info_out) { dca_set_error("%s: args or an output is NULL", who); return DCA_ERR_ARG; }
    if (args->selection != DCA_HOPFIELD_EXPLICIT && args->selection != DCA_HOPFIELD_LIKELIHOOD) { dca_set_error("%s: selection %d is neither explicit nor likelihood", who, args->selection); return DCA_ERR_ARG; }
    if (args->selection == DCA_HOPFIELD_EXPLICIT &&
        (args->num_attractive < 0 || args->num_attractive > 64 || args->num_repulsive < 0 || args->num_repulsive > 64)) {
        dca_set_error("%s: num_attractive %d or num_repulsive %d is outside 0 .. 64", who, args->num_attractive, args->num_repulsive);
        return DCA_ERR_ARG;
    }
    if (args->selection == DCA_HOPFIELD_LIKELIHOOD && (args->num_patterns < 1 || args->num_patterns > 128)) { dca_set_error("%s: num_patterns %d is outside 1 .. 128", who, args->num_patterns); return DCA_ERR_ARG; }
    if (!(args->tol > 0.0)) { dca_set_error("%s: tol %g must be > 0", who, args->tol); return DCA_ERR_ARG; }
    if (args->max_iterations < 1) { dca_set_error("%s: max_iterations %d < 1", who, args->max_iterations); return DCA_ERR_ARG; }
    if (!(pseudocount >= 0.0 && pseudocount < 1.0)) { dca_set_error("%s: pseudocount %g is outside [0, 1)", who, pseudocount); return DCA_ERR_ARG; }
    DCA_TRY(need_mf(ctx));
    return dca_mf_engine_hopfield_fit(ctx->mf, pseudocount, args, eigenvalues_out, gains_out, signs_out, patterns_out, residuals_out, info_out);
}
int dca_mf_model_kind(dca_ctx* ctx, int* kind_out)
{
    CHECK_CTX(ctx);
    if (!kind_out) return DCA_ERR_ARG;
    *kind_out = ctx->mf ? dca_mf_engine_model_kind(ctx->mf) : DCA_MF_MODEL_NONE;
    return DCA_OK;
}
int dca_mf_hopfield_couplings(dca_ctx* ctx, double* out)
{
    CHECK_CTX(ctx);
    if (!out) return DCA_ERR_ARG;
    DCA_TRY(need_mf(ctx));
    return dca_mf_engine_hopfield_couplings(ctx->mf, out);
}
int dca_hopfield_project(dca_ctx* ctx, const uint8_t* Q, int nq, int p, const double* patterns, double* out)
{
    CHECK_CTX(ctx);
    if (!patterns || !out) { dca_set_error("dca_hopfield_project: patterns or out is NULL"); return DCA_ERR_ARG; }
    if (p < 1) { dca_set_error("dca_hopfield_project: p %d < 1", p); return DCA_ERR_ARG; }
    if (Q && nq < 1) { dca_set_error("dca_hopfield_project: nq %d < 1", nq); return DCA_ERR_ARG; }
    if (!ctx->dX) { dca_set_error("dca_hopfield_project: dca_set_msa first"); return DCA_ERR_STATE; }
    // the patterns on all q states, a zero row for the gap, and no offsets: the projection kernel of the principal components
    const int L = ctx->L, q = ctx->q, qm = q - 1;
    std::vector<double> full((size_t)p * L * q, 0.0), zero(p, 0.0);
    for (int m = 0; m < p; ++m)
        for (int i = 0; i < L; ++i)
            memcpy(full.data() + ((size_t)m * L + i) * q, patterns + ((size_t)m * L + i) * qm, (size_t)qm * sizeof(double));
    return dca_pca_project_impl(ctx, Q, nq, p, full.data(), zero.data(), out);
}
int dca_dense_apply(dca_ctx* ctx, const double* A, int n, int ld, const double* V, int b, double* Y)
{
    CHECK_CTX(ctx);
    if (!A || !V || !Y || n < 1 || ld < n || b < 1 || b > 72) { dca_set_error("dca_dense_apply: a NULL array, n %d < 1, ld %d < n or b %d outside 1 .. 72", n, ld, b); return DCA_ERR_ARG; }
    return dca_dense_apply_impl(ctx, A, n, ld, V, b, Y);
}

int dca_spd_inverse(dca_ctx* ctx, const double* A, int n, double* Ainv_out)
{
    CHECK_CTX(ctx);
    if (!A || !Ainv_out || n <= 0) return DCA_ERR_ARG;
    const int np = (int)round_up((size_t)n, 64);
    std::vector<double> padded((size_t)np * np, 0.0);
    // the LOWER triangle of A is what is inverted (as LAPACK's 'L' routines read it): mirrored here, because the device
    // path reads both halves of the matrix
    for (int r = 0; r < n; ++r) {
        memcpy(padded.data() + (size_t)r * np, A + (size_t)r * n, (size_t)(r + 1) * sizeof(double));
        for (int c = 0; c < r; ++c) padded[(size_t)c * np + r] = A[(size_t)r * n + c];
    }
    for (int r = n; r < np; ++r) padded[(size_t)r * np + r] = 1.0;
    DevBuf<double> dA, dWork;
    HIP_TRY(dA.alloc(padded.size()));
    if (dWork.alloc(2 * padded.size()) != hipSuccess) { dca_set_error("out of device memory"); return DCA_ERR_NOMEM; }
    int info = 0;
    if (hipMemcpy(dA, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return DCA_ERR_HIP;
    double* dInv = nullptr;
    DCA_TRY(dca_spd_inverse_device(ctx, dA, np, dWork, &info, 1.0, &dInv));
    if (info != 0) { dca_set_error("matrix is not positive definite (pivot %d)", info); return DCA_ERR_NOT_SPD; }
    if (hipMemcpy(padded.data(), dInv, padded.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return DCA_ERR_HIP;
    for (int r = 0; r < n; ++r) memcpy(Ainv_out + (size_t)r * n, padded.data() + (size_t)r * np, (size_t)n * sizeof(double));
    return DCA_OK;
}

// ------------------------------------------------------------------ timing
int dca_set_profiling(dca_ctx* ctx, int on) { if (!ctx) return DCA_ERR_ARG; ctx->profiling = on != 0; ctx->profile_only.clear(); return DCA_OK; }
int dca_set_profiling_only(dca_ctx* ctx, const char* stage)
{
    if (!ctx) return DCA_ERR_ARG;
    ctx->profiling = stage && *stage;
    ctx->profile_only = stage ? stage : "";
    return DCA_OK;
}
int dca_reset_kernel_times(dca_ctx* ctx)
{
    CHECK_CTX(ctx);
    hipStreamSynchronize(ctx->stream);
    dca_flush_clocks(ctx);
    ctx->clocks.clear();
    return DCA_OK;
}
int dca_get_kernel_time(dca_ctx* ctx, const char* tag, double* ms_out, int* launches_out)
{
    CHECK_CTX(ctx);
    hipStreamSynchronize(ctx->stream);
    dca_flush_clocks(ctx);
    auto it = ctx->clocks.find(tag ? tag : "");
    if (ms_out) *ms_out = it == ctx->clocks.end() ? 0.0 : it->second.ms;
    if (launches_out) *launches_out = it == ctx->clocks.end() ? 0 : it->second.launches;
    return DCA_OK;
}

// ------------------------------------------------------------------ drop-in FFI
// plmdcaBackend.cpp:151-201: read + dedup, weights, initial x, L-BFGS; returns the
// parameter vector.  malloc/free are paired here (the reference mixes malloc/delete[]).
float* plmdcaBackend(unsigned short biomolecule, unsigned short num_site_states, const char* msa_file,
                     unsigned int seqs_len, float seqid, float lambda_h, float lambda_J,
                     unsigned int max_iteration, unsigned int num_threads, bool verbose)
{
    (void)num_threads;
    const int L = (int)seqs_len, q = (int)num_site_states;
    uint8_t* X = nullptr;
    int raw = 0;
    const int N = dca_read_msa_owned(msa_file, biomolecule, L, &X, &raw);       // one pass over the file
    if (N <= 0) { free(X); if (N == 0) dca_set_error("no sequences in %s", msa_file); return nullptr; }
    dca_ctx* ctx = nullptr;
    float* result = nullptr;
    dca_plm_stats st;
    memset(&st, 0, sizeof(st));
    const size_t P = dca_plm_num_params(L, q);
    if (dca_create(&ctx, 0, DCA_F32) != DCA_OK) { free(X); return nullptr; }
    const int rc_msa = dca_set_msa(ctx, X, N, L, q);
    free(X);
    if (rc_msa == DCA_OK &&
        dca_compute_weights(ctx, (double)seqid, DCA_F32) == DCA_OK &&
        dca_plm_configure(ctx, (double)lambda_h, (double)lambda_J, DCA_CARRY_CHUNKED, 0, 0, 0, 1) == DCA_OK &&
        dca_plm_init_x(ctx) == DCA_OK &&
        dca_plm_lbfgs_begin(ctx, (int)max_iteration, verbose ? 1 : 0) == DCA_OK &&
        dca_plm_lbfgs_iterate(ctx, max_iteration ? (int)max_iteration : 1 << 30, &st) == DCA_OK) {
        result = static_cast<float*>(malloc(P * sizeof(float)));
        if (!result) dca_set_error("out of host memory");
        else if (dca_plm_get_x(ctx, result, DCA_F32) != DCA_OK) { free(result); result = nullptr; }
    }
    if (verbose && result) {
        if (st.status == -1001) fprintf(stderr, "L-BFGS optimization completed\n");
        else { fprintf(stderr, "L-BFGS optimization terminated with status code = %d\n", st.status); fprintf(stderr, "fx = %f\n", st.fx); }
    }
    dca_destroy(ctx);
    return result;
}

void freeFieldsAndCouplings(void* h_and_J) { free(h_and_J); }

}  // extern "C"
