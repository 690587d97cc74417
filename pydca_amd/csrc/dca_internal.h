// Internal declarations shared by the translation units of libdca_hip.so.
// gfx950 (MI355X / CDNA4) only: wave = 64 lanes, 160 KiB LDS per CU, 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/dca_hip.h"
#include "potts_source.h"

void dca_set_error(const char* fmt, ...);

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            dca_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return DCA_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

// the message and code of a named entry: "<who>: <hipGetErrorString>", DCA_ERR_HIP; with nomem, hipErrorOutOfMemory becomes
// "<who>: out of device memory", DCA_ERR_NOMEM
#define HIP_TRY_AS_(expr, who, nomem)                                                                                     \
    do {                                                                                                                  \
        hipError_t _e = (expr);                                                                                           \
        if ((nomem) && _e == hipErrorOutOfMemory) { dca_set_error("%s: out of device memory", who); return DCA_ERR_NOMEM; } \
        if (_e != hipSuccess) { dca_set_error("%s: %s", who, hipGetErrorString(_e)); return DCA_ERR_HIP; }                 \
    } while (0)
#define HIP_TRY_AS(expr, who) HIP_TRY_AS_(expr, who, false)
#define HIP_TRY_AS_NOMEM(expr, who) HIP_TRY_AS_(expr, who, true)

#define HIP_PASS(expr) /* in a function that returns hipError_t */ \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return _e;                           \
    } while (0)

#define DCA_TRY(expr)                  \
    do {                               \
        int _rc = (expr);              \
        if (_rc != DCA_OK) return _rc; \
    } while (0)

#include "dev_buf.h"

#include "potts_plan.h"      // round_up, ceil_div and the launch geometry of the sequence-model kernels

// rows per pass of the set entries (dca_hamming_nearest, dca_three_site_values, dca_pca_project): DCA_NN_PASS, read per call; 32768, at most 2^20
static inline int dca_nn_pass_size()
{
    const char* e = getenv("DCA_NN_PASS");
    const long v = e ? atol(e) : 0;
    return v > 0 ? (int)(v < (1 << 20) ? v : 1 << 20) : 32768;
}

// number of XCDs on MI355X; workgroup b is observed to run on XCD b % 8
// (used for L2 locality only, never for correctness)
constexpr int kNumXcd = 8;

struct KernelClock {
    double ms = 0.0;
    int launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct PlmEngineBase;
struct MfEngine;
struct BmRun;
struct ArEngine;

#define DCA_SIDE_DEPTHS 3

struct dca_ctx {
    int device = 0;
    int precision = DCA_F32;
    hipStream_t stream = nullptr;

    // alignment (device): row-major bytes, row stride Ls (multiple of 128), zero padded
    int N = 0, L = 0, q = 0, Ls = 0;
    uint8_t* dX = nullptr;
    std::vector<uint8_t> hX;  // host copy, N x L, filled on demand by dca_host_msa()
    double* dLastScores = nullptr;   // most recent score vector (pair order), for dca_scores_order
    int nLastScores = 0;
    unsigned long long alignScratchBytes = 0;   // edge columns + pointer bits of the largest pass of the last dca_profile_align

    // weights
    bool have_weights = false;
    bool have_counts = false;
    uint32_t* dCounts = nullptr;
    double* dWd = nullptr;     // N doubles
    double meff = 0.0;
    unsigned long long weightsWork[2] = {0, 0};     // last weights launch: wave x 32-site groups compared / without the early exit
    int weightsPlanes = 0;                          // ... bit planes per group (5: q <= 32, 3: q <= 8)

    // scratch scalars: device slots + pinned host mirror
    double* dScal = nullptr;
    double* hScal = nullptr;

    PlmEngineBase* plm = nullptr;
    MfEngine* mf = nullptr;
    BmRun* bm = nullptr;          // Boltzmann-learning run in progress (boltzmann.hip)
    ArEngine* ar = nullptr;       // autoregressive model (ardca.hip)

    // native communicator (comm_rccl.cpp): an RCCL communicator whose collectives run on `stream`
    void* comm = nullptr;
    std::atomic<bool> comm_aborted{false};      // dca_comm_abort ran (from a watchdog thread): the communicator is already released
    int comm_rank = 0, comm_world = 0;
    void* commStage = nullptr;        // pieces received by the direct-exchange reduce-scatter ((world - 1) slices)
    size_t commStageBytes = 0;

    bool profiling = false;
    std::string profile_only;      // non-empty: only the stage of this name is clocked (bench.py's timed region: the roofline kernel alone)
    std::map<std::string, KernelClock> clocks;
};

// RAII-less helpers for bracketing a kernel with events on ctx->stream
struct ScopedKernelClock {
    dca_ctx* ctx;
    KernelClock* kc = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedKernelClock(dca_ctx* c, const char* tag) : ctx(c) {
        if (!c->profiling) return;
        if (!c->profile_only.empty() && c->profile_only != tag) return;
        kc = &c->clocks[tag];
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { kc = nullptr; return; }
        hipEventRecord(a, c->stream);
    }
    ~ScopedKernelClock() {
        if (!kc) return;
        hipEventRecord(b, ctx->stream);
        kc->pending.emplace_back(a, b);
        kc->launches += 1;
    }
};
void dca_flush_clocks(dca_ctx* ctx);

// host copy of the alignment (N x L), fetched from the device the first time it is needed
const uint8_t* dca_host_msa(dca_ctx* ctx);
// keeps a device copy of a score vector for dca_scores_order
int dca_remember_scores(dca_ctx* ctx, const double* dScores, int n);
// rank.hip: indices of a device score vector in descending order, ties by ascending index (stable)
int dca_scores_order_device(dca_ctx* ctx, const double* dScores, int n, int32_t* order_out /* host */);

// n doubles computed on the device by compute(d) (an int (double*) that reports its own errors), copied to the host `out` once
// the stream has drained.  A failing copy reads "<who>: ..."; with nomem_who a failing allocation reads "<nomem_who>: out of
// device memory" and is DCA_ERR_NOMEM.
template <class F>
int dca_download_doubles(dca_ctx* ctx, size_t n, double* out, const char* who, F&& compute, const char* nomem_who = nullptr)
{
    DevBuf<double> d;
    const hipError_t ea = d.alloc(n);
    if (ea != hipSuccess && nomem_who) {
        (void)hipGetLastError();
        dca_set_error("%s: out of device memory", nomem_who);
        return DCA_ERR_NOMEM;
    }
    HIP_TRY(ea);
    DCA_TRY(compute(d.get()));
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    HIP_TRY_AS(hipMemcpy(out, d, n * sizeof(double), hipMemcpyDeviceToHost), who);
    return DCA_OK;
}

// ---- weights.hip
// part / parts: this context counts the tile pairs  t % parts == part  of the upper triangle (1 / parts of the N^2 L / 2
// comparisons, evenly spread); finish = false leaves the partial counts in ctx->dCounts for the caller to sum
int dca_weights_compute(dca_ctx* ctx, double seqid, int compare_precision, int part = 0, int parts = 1, bool finish = true);
int dca_weights_finish(dca_ctx* ctx);     // w = 1 / count, Meff from ctx->dCounts

// ---- comm_rccl.cpp
int dca_comm_unique_id_impl(const char* rccl_path, void* id128);
int dca_comm_init_impl(dca_ctx* ctx, const char* rccl_path, const void* id128, int world, int rank);
void dca_comm_destroy_impl(dca_ctx* ctx);
int dca_comm_abort_impl(dca_ctx* ctx);
int dca_comm_info_impl(dca_ctx* ctx, int* world, int* rank);
int dca_comm_p2p_begin(dca_ctx* ctx);
int dca_comm_p2p_send(dca_ctx* ctx, const void* buf, size_t count, int dtype, int peer);
int dca_comm_p2p_recv(dca_ctx* ctx, void* buf, size_t count, int dtype, int peer);
int dca_comm_p2p_end(dca_ctx* ctx);
int dca_comm_native(dca_ctx* ctx, int op, void* buf, size_t count, int dtype, bool direct = false);   // direct: grouped send / recv + local sum
int dca_comm_native_reduce(dca_ctx* ctx, void* vec, size_t count, int dtype, double* scalar_dev);
int dca_comm_native_sum_u32(dca_ctx* ctx, uint32_t* buf, size_t count);

// ---- plm engine
struct PlmEngineBase {
    virtual ~PlmEngineBase() {}
    virtual int configure(double lambda_h, double lambda_J, int carry_mode, int chunk, int warmup,
                          int halo, int add_reg) = 0;
    virtual int configure_strips(double lambda_h, double lambda_J, int carry_mode, int chunk, int warmup) = 0;   // column-strip decomposition over ctx->comm
    virtual int init_x() = 0;
    virtual int set_x(const void* x, int dtype) = 0;
    virtual int get_x(void* x, int dtype) = 0;
    virtual int get_g(void* g, int dtype) = 0;
    virtual int gradient(double* fx_out) = 0;
    virtual int lbfgs_begin(int max_iterations, int verbose) = 0;
    virtual int lbfgs_iterate(int iterations, dca_plm_stats* st) = 0;
    virtual void lbfgs_end() = 0;       // abandons the optimisation in progress (x, g stay as they are)
    virtual int scores(int apc, double* out) = 0;
    virtual int di_scores(const double* reg_fi, int apc, double* out) = 0;
    virtual int pair_couplings(const int* pairs, int npairs, int shift, double* out) = 0;
    // the current x as a Potts source (energy.hip, pll.hip, sample.hip, sample_conditional.hip, ascent.hip, ais.hip); column strips gather x first, as scores() does.
    // one_gpu_only (AIS, conditional sampling, ascent): DCA_ERR_STATE under column strips, vector sharding, a reduce / comm hook or a native-comm mode instead
    virtual int potts_source(PottsSource* out, bool one_gpu_only) = 0;
    // the device x a Boltzmann-learning run updates in place; DCA_ERR_STATE (with the reason) unconfigured, during an L-BFGS
    // run, under column strips, vector sharding, a reduce / comm hook or a native-comm mode
    virtual int bm_source(void** dx) = 0;
    // the device x for a transformation in place (dca_plm_zero_sum_gauge): dca_plm_set_x's rules (configured; an L-BFGS run in
    // progress continues from the new x), on one GPU only as bm_source
    virtual int transform_source(void** dx) = 0;
    virtual int set_vector_sharding(int rank, int world, dca_comm_hook hook, void* user) = 0;
    dca_reduce_hook hook = nullptr;
    void* hook_user = nullptr;
    virtual void weights_changed() = 0;            // dca_compute_weights* / dca_set_weights ran: configure again, exchange scheme kept
    virtual int set_native_comm(int mode) = 0;     // 0 off, 1 all-reduce of g and fx, 2 sharded optimiser vectors, 3 the same by direct exchange
    virtual bool configured_for_comm() const = 0;  // configured: its slices follow a communicator (an unconfigured engine re-cuts them in configure)
    int native_mode = 0;                           // ... through ctx->comm (RCCL) on the context's stream
};
PlmEngineBase* dca_make_plm_engine(dca_ctx* ctx);

// ---- scoring.hip
// FN of (q-1)x(q-1) blocks.  Source kind 0: packed plm vector of element type `dtype`
// (DCA_F32/DCA_F64); 1: dense n x n double couplings with leading dimension ld.
int dca_fn_scores(dca_ctx* ctx, const void* src, int src_kind, int dtype, int L, int q, int ld,
                  int apc, double* dScoresOut /* device, pairs */);

int dca_di_scores(dca_ctx* ctx, const void* src, int src_kind, int dtype, const double* dRegFi, int L, int q, int ld,
                  int apc, double* dScoresOut /* device, pairs */);

int dca_pair_blocks(dca_ctx* ctx, const void* src, int src_kind, int dtype, int L, int q, int ld, const int* pairs, int npairs,
                    int shift, double* out /* host */);

// ---- energy.hip : Potts energies of host query rows (n x L codes < q) and single-mutant scans of a wild type (L codes).
// The model: a PottsSource (potts_source.h).  out: host.
int dca_potts_energies(dca_ctx* ctx, const PottsSource& ps, const uint8_t* X, int n, double* out);
int dca_potts_mutation_scan(dca_ctx* ctx, const PottsSource& ps, const uint8_t* wildtype, double* out /* L*q */);

// ---- pll.hip : site conditionals and pseudo-log-likelihoods of host query rows under the same sources (dca_plm_pseudo_likelihood
// semantics).  site_out (n*L) and cond_out (n*L*q) may be NULL; all outputs on the host.
int dca_potts_pseudo_likelihood(dca_ctx* ctx, const PottsSource& ps, const uint8_t* X, int n, double* pll_out, double* site_out,
                                double* cond_out);

// The pair stage of dca_potts_energies on device codes QT[s * NqS + k] (k < nq, NqS a multiple of 128): slab g of query k at
// dSlabs[g * NqS + k], g < dca_energy_slab_count(ps).  E(k) = sum_i h_i (ascending i) + sum_g slab (ascending g) is then
// bit for bit what dca_potts_energies returns for those codes.
int dca_energy_slab_count(const PottsSource& ps);
hipError_t dca_energy_pairs_device(dca_ctx* ctx, const PottsSource& ps, const uint8_t* dQT, int nq, int NqS, double* dSlabs);

// ---- sample.hip : Gibbs sampling of n chains (one launch per sweep) under the same sources.  initial / out: host, n x L.
int dca_potts_sample(dca_ctx* ctx, const PottsSource& ps, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep,
                     double beta, const uint8_t* initial /* host n*L or NULL */, uint8_t* out /* host n*L */);

// ---- sample_conditional.hip : the same with every site outside free_sites (num_free strictly ascending indices) clamped to
// `initial` (dca_plm_sample_conditional semantics; all arguments checked here)
int dca_potts_sample_conditional(dca_ctx* ctx, const PottsSource& ps, int n, int sweeps, uint64_t seed, uint64_t first_chain,
                                 uint64_t first_sweep, double beta, const int32_t* free_sites, int num_free,
                                 const uint8_t* initial /* host n*L */, int random_start, uint8_t* out /* host n*L */);

// DCA_ERR_ARG unless free_sites holds F indices of [0, L), strictly ascending (F in [0, L]); `who` opens the message
int dca_check_free_sites(const int32_t* free_sites, int F, int L, const char* who);

// ---- interaction.hip : inter-protein energies of host rows XA (nA x split) and XB (nB x (L - split)) in G groups
// (dca_plm_interaction_energies semantics; all arguments checked here).  out: host.
int dca_potts_interaction_energies(dca_ctx* ctx, const PottsSource& ps, int split, const uint8_t* XA, int nA, const uint8_t* XB, int nB,
                                   const int32_t* offsets_a, const int32_t* offsets_b, int G, int gauge, double* out);

// ---- ascent.hip : greedy ascent of host rows X (n x L codes < q) to local maxima of E over the free sites (dca_plm_ascend
// semantics; all arguments checked here).  All outputs on the host; gain_out, path_out and path_gain_out may be NULL.
int dca_potts_ascend(dca_ctx* ctx, const PottsSource& ps, const uint8_t* X, int n, const int32_t* free_sites, int num_free, int max_steps,
                     double min_gain, uint8_t* out, int32_t* steps_out, uint8_t* converged_out, double* gain_out, int32_t* path_out,
                     double* path_gain_out);

// Philox4x32-10 of the samplers (sample.hip, ais.hip): key = (seed lo, seed hi), counter = (chain, sweep, site, tag), each
// word the value mod 2^32; U = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53.  Tags: 0 Gibbs draw, 1 random start, 2 AIS start,
// 3 ancestral draw of the autoregressive sampler (ardca.hip, counter (chain, 0, site, 3)), 4 the start vectors of the PCA
// (pca.hip), 5 the exchange decision of replica exchange (tempered.hip, counter (ladder, round, lower level, 5)).
static __host__ __device__ __forceinline__ void philox4x32_10(const uint32_t in[4], const uint32_t k[2], uint32_t out[4])
{
    uint32_t c0 = in[0], c1 = in[1], c2 = in[2], c3 = in[3], k0 = k[0], k1 = k[1];
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

static __device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t chain, uint64_t sweep, int site, uint32_t tag)
{
    const uint32_t ctr[4] = {(uint32_t)chain, (uint32_t)sweep, (uint32_t)site, tag};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    return (double)((uint64_t)(w[0] >> 5) * 67108864ull + (w[1] >> 6)) * 0x1.0p-53;
}

// Device-resident chains of the sampler: site-major codes st[s * nS + c], nS = n rounded up to 64 (the chains past n are
// swept too and never read).  dca_chains_start: tag-1 random starts of chains first_chain + c, or the host rows `initial`
// (n x L codes < q, checked by the caller).  dca_chains_sweeps: `sweeps` launches numbered first_sweep.., one per sweep, under
// the tag "sample"; with dBase (L x q device doubles) the sweeps draw from the AIS interpolation h0 + bk * (u - h0) instead
// (beta unused); with dBetas (nS device doubles) chain c sweeps under its own dBetas[c] in the place of beta (tempered.hip).
// dca_chains_read: the n x L rows to the host (synchronises).  Any nS that is a multiple of 64 works (ais.hip and tempered.hip
// use multiples of 128, the energy kernels' stride: `stride` of dca_chains_start).
struct DcaChains { int n = 0, L = 0, nS = 0; DevBuf<uint8_t> dState; };
int dca_chains_start(dca_ctx* ctx, DcaChains* ch, int n, int L, int q, uint64_t seed, uint64_t first_chain, const uint8_t* initial,
                     int stride = 64);
int dca_chains_sweeps(dca_ctx* ctx, const DcaChains& ch, const PottsSource& ps, int sweeps, uint64_t seed, uint64_t first_chain,
                      uint64_t first_sweep, double beta, const double* dBase = nullptr, double bk = 0.0,
                      const double* dBetas = nullptr);
int dca_chains_read(dca_ctx* ctx, const DcaChains& ch, uint8_t* out);

// ---- ais.hip : annealed importance sampling of log Z under the same sources (dca_plm_ais / dca_mf_ais; arguments checked here)
int dca_potts_ais(dca_ctx* ctx, const PottsSource& ps, const dca_ais_args* args, double* log_weights_out, double* log_z0_out,
                  uint8_t* chains_out);
double dca_ais_log_z0(const double* h0, int L, int q);    // host, L x q base fields

// ---- tempered.hip : replica-exchange Gibbs sampling on a temperature ladder under the same sources (dca_plm_sample_tempered /
// dca_mf_sample_tempered; arguments checked here)
int dca_potts_sample_tempered(dca_ctx* ctx, const PottsSource& ps, const dca_pt_args* args, uint8_t* out, int32_t* levels_out,
                              double* energies_out, uint64_t* attempts_out, uint64_t* accepts_out, double* energy_trace_out,
                              int* rounds_out);

// ---- boltzmann.hip : Boltzmann machine learning of the plm vector (dca_plm_bm_*).  The run lives in ctx->bm; dca_bm_free ends
// it (alignment, weights, configure, L-BFGS begin, engine release, destroy).  x: the plm engine's device vector (PlmEngineBase::
// bm_source), looked up again on every call.
struct BmRun;
int dca_bm_begin_impl(dca_ctx* ctx, void* dx, int dtype, const dca_bm_args* args);
int dca_bm_iterate_impl(dca_ctx* ctx, void* dx, int iterations, dca_bm_record* records_out);
int dca_bm_freqs_impl(dca_ctx* ctx, int which, double* fi_out, double* fij_out);
int dca_bm_chains_impl(dca_ctx* ctx, uint8_t* out);
void dca_bm_free(dca_ctx* ctx);

// ---- decimation.hip : the mask of a Boltzmann-learning run, the decimation of its couplings (dca_plm_bm_set_mask / get_mask /
// decimate; the run's checks here) and the zero-sum gauge of the plm vector dx (dca_plm_zero_sum_gauge)
int dca_bm_set_mask_impl(dca_ctx* ctx, void* dx, const uint8_t* mask);
int dca_bm_get_mask_impl(dca_ctx* ctx, uint8_t* out);
int dca_bm_decimate_impl(dca_ctx* ctx, void* dx, long long remove, double* scores_out, dca_bm_decimation* info);
bool dca_bm_has_removed(const dca_ctx* ctx);       // a run whose mask has removed elements
int dca_zero_sum_gauge_impl(dca_ctx* ctx, void* dx, int dtype);

// the chains' unweighted frequencies by the UPDATE = false instantiations of the statistics kernels (exact integer LDS
// histograms): dGi (L*q) and dGij (pairs*q*q, pair order), device.  Under the tag "bm_stats"; no run is needed or touched.
hipError_t dca_bm_count_chains(dca_ctx* ctx, const DcaChains& ch, int q, double* dGi, double* dGij);

// ---- distance.hip / set_stats.hip : a sequence set against the alignment (dca_hamming_nearest, dca_sequence_statistics,
// dca_alignment_statistics; arguments checked by the callers in capi.cpp).  Q == NULL in dca_set_statistics_impl: the alignment's
// weighted frequencies go to fi_out / fij_out instead of the set's.
int dca_hamming_nearest_impl(dca_ctx* ctx, const uint8_t* Q, int nq, const uint8_t* R, int nr, bool skip_same, int32_t* dist_out,
                             int32_t* index_out, uint64_t* hist_out);
int dca_set_statistics_impl(dca_ctx* ctx, const uint8_t* Q, int nq, double* fi_out, double* fij_out, dca_set_comparison* cmp_out);

// ---- redundancy.hip : the greedy redundancy filter and the identity clusters (dca_identity_filter, dca_identity_clusters;
// the state, n, T and the NULL outputs checked in capi.cpp, the codes and the order here)
int dca_identity_filter_impl(dca_ctx* ctx, const uint8_t* X, int n, int T, const int32_t* order, uint8_t* keep_out, int32_t* rep_out,
                             dca_filter_info* info);
int dca_identity_clusters_impl(dca_ctx* ctx, const uint8_t* X, int n, int T, int32_t* label_out, int32_t* degree_out,
                               dca_cluster_info* info);

// ---- align.hip : profile alignment, one lane per query (dca_profile_align, dca_sw_scores_device; every argument checked in capi.cpp)
int dca_profile_align_impl(dca_ctx* ctx, const int32_t* match, int Lp, int A, const int32_t* del_open, const int32_t* del_extend,
                           int ins_open, int ins_extend, int mode, const uint8_t* seqs, const int64_t* offsets, int n,
                           int32_t* score_out, int32_t* residue_at_out, unsigned long long* scratch_bytes_out);

// ---- three_site.hip : three-site connected correlations of the alignment (Q == NULL, quantised weights) or of a set, at listed
// elements and as a scan for the K strongest (dca_three_site_values, dca_three_site_scan; arguments checked in capi.cpp except
// the elements and the codes)
int dca_three_site_values_impl(dca_ctx* ctx, const uint8_t* Q, int nq, const int32_t* elements, int T, uint64_t* count_out,
                               uint64_t* denom_out, double* f3_out, double* c3_out);
int dca_three_site_scan_impl(dca_ctx* ctx, const uint8_t* Q, int nq, int K, int skip_state, int32_t* elements_out, double* c3_out,
                             double* f3_out, int* found);

// ---- pca.hip : principal components of the reweighted alignment and projections onto them (dca_pca_fit, dca_pca_project;
// arguments checked in capi.cpp except the codes)
int dca_pca_fit_impl(dca_ctx* ctx, int k, double tol, int max_iterations, uint64_t seed, double* eigenvalues_out,
                     double* components_out, double* offsets_out, double* residuals_out, double* total_variance_out,
                     int* iterations_out, int* converged_out);
int dca_pca_project_impl(dca_ctx* ctx, const uint8_t* Q, int nq, int k, const double* components, const double* offsets,
                         double* proj_out);

// the small block algebra of the fit for hopfield.hip: pca.hip's init, Gram + sum and rotate kernels as the fit launches them
// (blocks are rows x b row-major; dGpart holds dca_pca_small_chunks(rows) * ba * bb doubles)
int dca_pca_small_chunks(int rows);
int dca_pca_small_init(dca_ctx* ctx, const char* who, double* dV, int rows, int b, uint64_t seed);
int dca_pca_small_gram(dca_ctx* ctx, const char* who, const double* dA, int ba, const double* dB, int bb, int rows, bool diag,
                       double* dGpart, double* dOut);
int dca_pca_small_rotate(dca_ctx* ctx, const char* who, const double* dA, const double* dT1, const double* dB, const double* dT2, int rows,
                         int b, double* dOut);

// ---- hopfield.hip : the kernels of the Hopfield-Potts fit (dca_mf_engine_hopfield_fit drives them)
int dca_hp_factor(dca_ctx* ctx, const double* dC, int L, int qm, int ld, double* dRinv);       // L * qm * qm doubles
int dca_hp_whiten(dca_ctx* ctx, double* dC, int L, int qm, int ld, const double* dRinv);                   // in place
int dca_hp_apply(dca_ctx* ctx, const double* dA, int n, int ld, const double* dV, int b, double* dY, double* dPart);
int dca_hp_eigs(dca_ctx* ctx, const double* dA, int n, int ld, int k, double tol, int max_iterations, uint64_t seed, double* theta_out,
                double* res_out, DevBuf<double>* dV, int* iterations_out, int* converged_out);
int dca_hp_residuals(dca_ctx* ctx, const double* dA, int n, int ld, const double* dV, int b, const double* lambda, double* res_out);
int dca_hp_assemble(dca_ctx* ctx, const double* xi, const int32_t* sign, int p, int n, double* dJ, int ld);
int dca_dense_apply_impl(dca_ctx* ctx, const double* A, int n, int ld, const double* V, int b, double* Y);

int dca_di_from_arrays_impl(dca_ctx* ctx, const double* couplings, int layout, const double* reg_fi, int L, int q,
                            double* fields_out, double* di_out, const double* fields_in = nullptr);

// ---- ardca.hip : the autoregressive model (dca_ar_*).  Freed with the alignment; unconfigured when the weights change.
ArEngine* dca_make_ar_engine(dca_ctx* ctx);
void dca_free_ar_engine(ArEngine*);
void dca_ar_engine_weights_changed(ArEngine*);
// for ar_epistasis.hip: the engine's device x and its (L, q) (false before the first configure), and cond_l(b) of one host row
// (L codes, model order) into dCond (device, L*q) through the logits kernel
bool dca_ar_engine_model(ArEngine*, const double** dx, int* L, int* q);
int dca_ar_engine_conditionals(ArEngine*, const uint8_t* row, double* dCond);

// ---- mf engine
struct MfEngine;
MfEngine* dca_make_mf_engine(dca_ctx* ctx);
void dca_free_mf_engine(MfEngine*);
int dca_mf_engine_site_freqs(MfEngine*, double* fi_out);
int dca_mf_engine_pair_freqs(MfEngine*, double* fij_out);
int dca_mf_engine_corr(MfEngine*, double theta, double* corr_out);
int dca_mf_engine_couplings(MfEngine*, double* out);
int dca_mf_engine_scores(MfEngine*, int apc, double* out);
int dca_mf_engine_di(MfEngine*, int apc, double* out);
int dca_mf_engine_fields(MfEngine*, double* out);
void dca_mf_engine_set_hook(MfEngine*, dca_reduce_hook hook, void* user);
void dca_mf_engine_set_native(MfEngine*, bool on);
int dca_mf_engine_set_row_window(MfEngine*, int first, int count);   // count < 0: all rows
void dca_mf_engine_invalidate(MfEngine*);      // weights changed: counts, frequencies, C and J are recomputed on demand
int dca_mf_engine_pair_couplings(MfEngine*, const int* pairs, int npairs, int shift, double* out);
// the mean-field model as a Potts source: J = -inv(C), h = the fields of dca_mf_engine_fields in a device buffer allocated here
// (*dH_owned: it must outlive the use of the source)
int dca_mf_engine_potts_source(MfEngine*, PottsSource* out, DevBuf<double>* dH_owned);
// data statistics of a Boltzmann-learning run from this engine's weighted counts (dca_plm_bm_begin): device outputs
// fi (L*q) = (1 - lambda) * f_i + lambda / q and fij (pairs*q*q, pair order, gap included) = (1 - lambda) * f_ij + lambda / q^2
int dca_mf_engine_bm_freqs(MfEngine*, double lambda, double* dFi, double* dFij);
// the Hopfield-Potts fit (dca_mf_hopfield_fit; arguments checked in capi.cpp): afterwards the engine's J is the Hopfield-Potts one
int dca_mf_engine_hopfield_fit(MfEngine*, double theta, const dca_hopfield_args* args, double* eigenvalues_out, double* gains_out,
                               int32_t* signs_out, double* patterns_out, double* residuals_out, dca_hopfield_info* info_out);
int dca_mf_engine_model_kind(const MfEngine*);
int dca_mf_engine_hopfield_couplings(MfEngine*, double* out);

// ---- cholinv.hip : scale * inverse of an SPD matrix on the device (f64 MFMA)
// dA: n x n row-major (ld = n), n multiple of 64; destroyed (holds the triangular factor's inverse afterwards).
// dWork: >= 2*n*n doubles; *result points into it (its second half): scale * inv(A), full and bit-symmetric.
// info_out: 0 ok, >0 first non-positive pivot (1-based).
int dca_spd_inverse_device(dca_ctx* ctx, double* dA, int n, double* dWork, int* info_out, double scale, double** result);

// ---- host_io.cpp
int dca_read_msa_impl(const char* path, int biomolecule, int L, uint8_t* out, int capacity, int* raw_count);
int dca_read_msa_owned(const char* path, int biomolecule, int L, uint8_t** rows /* malloc'd, caller frees */, int* raw_count);   // one pass, no capacity
int dca_count_msa_lines_impl(const char* path);
int dca_encode_sequences_impl(const char* seqs, const int* offsets, int nseq, int biomolecule, int table, int L, uint8_t* out,
                              int* bad_record);
