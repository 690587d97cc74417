// plmDCA on MI355X: objective + "gradient" of the reference (PlmDCA::gradient,
// pydca/plmdca/plmdca_numerics.cpp:436-607) and the L-BFGS driver the backend runs
// (pydca/plmdca/plmdcaBackend.cpp:47-146, lbfgs/lib/lbfgs.cpp:248-644, :815-1004,
// :1128-1295), re-designed for gfx950.
//
// One evaluation =
//   expand : packed x -> symmetric table  W[(j,b)][(i,a)]              (HBM-bound, P floats in)
//   logits : S[n][(i,a)] = sum_j W[(j,x_nj)][(i,a)]                     (register gather, source row selected by M0)
//   softmax: per site, scan over n with the reference's carried-over probabilities,
//            R[n][(i,a)] = w_n (p_ni(a) - delta(a,x_ni)),  fx -= w_n log p_ni(x_ni)   (lanes = sites)
//   scatter: G[(j,b)][(i,a)] = sum_n [x_nj = b] R[n][(i,a)]             (LDS gather, destination sum selected by M0)
//   fold   : g = 2 lambda x + G + G^T in the packed layout, regulariser value
// The two N*L^2*q stages (logits, scatter) are gathers with a wave-uniform row index: lanes are
// columns and the VGPR index mode picks the register (generated inner blocks, tools/gen_plm_asm.py).
// They are bound on chip (fp32 adds + one SALU per 512-byte row piece); see DESIGN.md section 4.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "dca_internal.h"
#include "more_thuente.h"
#include "vec_kernels.h"
#include "plm_plan.h"
#include "plm_stages.h"
#include "lbfgs_kernels.h"

namespace {

static_assert(kPlanXcds == kNumXcd, "the planner deals strips to this many XCDs");

#ifdef DCA_ROUND_ABLATE
// ANALYSIS BUILD ONLY (make ablate -> lib/libdca_hip_ablate.so; the shipped library has no such switch): the float64 engine
// rounds the output of selected stages to float32, DCA_ROUND_F32_STAGES = bit mask (1 W, 2 S, 4 R, 8 G, 16 g, 32 x, 64 d).
// Rounding a stage's OUTPUT is a lower bound on what computing that stage in float32 would do to the result; used to
// decide which mixed-precision pipelines can keep protocol P3 (tests/analysis/mixed_precision_table.py).
__global__ void round_to_f32_kernel(double* __restrict__ p, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (double)(float)p[i];
}
inline int round_stage_mask() { const char* e = getenv("DCA_ROUND_F32_STAGES"); return e ? atoi(e) : 0; }
#define DCA_ROUND_STAGE(bit, ptr, count)                                                                             \
    do {                                                                                                             \
        if constexpr (sizeof(T) == 8)                                                                                \
            if (round_stage_mask() & (bit))                                                                          \
                hipLaunchKernelGGL(round_to_f32_kernel, dim3(2048), dim3(256), 0, ctx->stream, reinterpret_cast<double*>(ptr), (size_t)(count)); \
    } while (0)
#else
#define DCA_ROUND_STAGE(bit, ptr, count) do { } while (0)
#endif

template <typename T>
struct PlmEngine : PlmEngineBase {
    dca_ctx* ctx;
    int N, L, q, Ls;
    double lambda_h = 0, lambda_J = 0;
    int carry_mode = DCA_CARRY_CHUNKED, halo = 0, add_reg = 1;
    bool configured = false;
    PlmPlan plan;                  // the launch geometry and array shapes (plm_plan.h), made by configure
    PlmKnobs knobs;                // ... under these tuning knobs, read from the environment by configure

    T *dx = nullptr, *dg = nullptr, *dxp = nullptr, *dgp = nullptr, *dd = nullptr;
    T* dS[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    T* dY[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    T *dWt = nullptr, *dSR = nullptr, *dR = nullptr, *dG = nullptr, *dw = nullptr;
    LbfgsDev* dLb = nullptr;       // optimiser scalars on the device (two-loop recursion)
    uint16_t* dXL = nullptr;
    uint16_t* dXT2 = nullptr;
    PairIJ* dPairs = nullptr;
    double *dFxPart = nullptr, *dRegPart = nullptr, *dVecPart = nullptr;
    double *dColPart = nullptr, *dColSum = nullptr;      // float64 mode: column sums of R in double-double
    double* dColChunk = nullptr;                         // ... q = 5: per scan chunk, from the softmax kernel
    // Column-strip decomposition (native_mode 4, configure_strips): this rank holds the COLUMNS of sites [cS0, cS1) of W, S, R
    // and G (re-based to column 0; Cs is the window's stride), walks all sequences, and owns the packed parameters
    // [oLo, oHi): the pairs (i, j) whose first site it holds (rank 0 the fields too).  Without it the window is everything.
    bool stripRequested = false, strips = false, stripEmulate = false;
    int sWorld = 1, sRank = 0;
    T *dGrecv = nullptr, *dXsend = nullptr, *dXrecv = nullptr;
    // every device buffer of the engine, named here once: freeall() releases and clears them through this list
    template <typename F> void each_buffer(F f)
    {
        f(dx); f(dg); f(dxp); f(dgp); f(dd);
        for (int i = 0; i < 5; ++i) { f(dS[i]); f(dY[i]); }
        f(dWt); f(dSR); f(dR); f(dG); f(dw); f(dLb); f(dXL); f(dXT2); f(dPairs); f(dFxPart); f(dRegPart); f(dVecPart);
        f(dColPart); f(dColSum); f(dColChunk); f(dGrecv); f(dXsend); f(dXrecv);
    }
    int strip_cs(int r) const { return plm_strip_cs(plan.siteB, q, r); }
    size_t owned_lo(int r) const { return plm_owned_lo(plan.siteB, L, q, r); }
    size_t owned_hi(int r) const { return plm_owned_hi(plan.siteB, L, q, r); }
    bool lbfgs_alloc = false;
    bool deferFx = false, fxPending = false;      // fx of the last evaluation still lies in its partial sums (eval_scalars finishes it)
    // vector sharding (dca_plm_set_vector_sharding): this rank's slice [vlo, vlo + vn) of every P-vector;
    // collectives run over Ppad = world * slice elements.  Unsharded: vlo = 0, vn = Ppad = P.
    size_t vlo = 0, vn = 0, Ppad = 0;
    dca_comm_hook comm = nullptr;
    void* comm_user = nullptr;
    int comm_rank = 0, comm_world = 0;      // of the hook-driven sharding, so that configure() can cut the slices again

    // optimiser state (resumable)
    struct {
        bool begun = false, finished = false;
        int status = 0, k = 1, end = 0, iters = 0, evals = 0, max_iterations = 0, verbose = 0;
        double fx = 0, step = 0, xnorm = 0, gnorm = 0, seconds = 0;
        double last_step = 0;                 // step length the last completed iteration accepted (lbfgs_progress_t's `step`)
        double dginit = 0;                    // g.d of the current search direction
        bool dginit_on_device = false;        // ... still in dScal[kSlotDginit]: read with the next evaluation's scalars
        // the fused step pass (lbfgs_dir_trial_expand_kernel) ran for the pending direction: dxp and W hold x + 1 * d.  Whatever
        // rewrites x, d or W outside the line search's first trial clears it (the resets of `o` do so by themselves)
        bool trial_ready = false;
    } o;

    explicit PlmEngine(dca_ctx* c) : ctx(c), N(c->N), L(c->L), q(c->q), Ls(c->Ls) {}

    template <typename U> int dalloc(U** p, size_t n)
    {
        HIP_TRY(dca_dev_malloc(reinterpret_cast<void**>(p), std::max<size_t>(n, 1) * sizeof(U)));
        return DCA_OK;
    }
    void freeall() { each_buffer([](auto*& p) { dca_dev_free(p); p = nullptr; }); }
    ~PlmEngine() override { freeall(); }

    // the engine's copy of the weights (dw, made by configure) is stale: everything answers DCA_ERR_STATE until the caller
    // configures again; hooks, native mode and vector sharding are kept (configure re-applies them)
    void weights_changed() override { configured = false; o = decltype(o)(); }

    int configure(double lh, double lJ, int cmode, int chunk_, int warm_, int halo_, int add_reg_) override
    {
        if (q != 21 && q != 5) { dca_set_error("plmDCA kernels are built for q = 21 (protein) and q = 5 (RNA); got %d", q); return DCA_ERR_ARG; }
        if (!ctx->have_weights) { dca_set_error("weights must be computed or set before dca_plm_configure"); return DCA_ERR_STATE; }
        if (halo_ < 0 || halo_ >= N) { dca_set_error("halo out of range"); return DCA_ERR_ARG; }
        if (L > 65535) { dca_set_error("L too large"); return DCA_ERR_ARG; }
        // from here on members are overwritten: an engine that fails below must not keep running with the half-updated window
        // (arrays, siteB and the receive offsets would still be sized for the old one)
        configured = false;
        lambda_h = lh; lambda_J = lJ; carry_mode = cmode; halo = halo_; add_reg = add_reg_;
        // the column window first: the scan's chunking below depends on how many sites this rank walks
        strips = stripRequested && ctx->comm && ctx->comm_world > 1;
        stripRequested = false;
        sWorld = strips ? ctx->comm_world : 1;
        sRank = strips ? ctx->comm_rank : 0;
#ifdef DCA_ROUND_ABLATE
        // ANALYSIS BUILD ONLY: DCA_STRIP_EMULATE=rank,world cuts the column window of that rank WITHOUT a communicator and
        // skips the two exchanges -- the evaluation's results are then wrong, its kernel times are those of one rank of the
        // column-strip decomposition (tools/time_eval.py under the analysis library)
        stripEmulate = false;
        if (const char* e = getenv("DCA_STRIP_EMULATE")) {
            int er = 0, ew = 1;
            if (sscanf(e, "%d,%d", &er, &ew) == 2 && ew > 1 && er >= 0 && er < ew) { strips = true; stripEmulate = true; sRank = er; sWorld = ew; }
        }
#endif
        if (sWorld > kMaxStripRanks || (strips && sWorld > L)) { dca_set_error("column strips: too many ranks for %d sites", L); return DCA_ERR_ARG; }
        if (strips && (halo || hook || comm)) { dca_set_error("column strips take the whole alignment and no hooks"); return DCA_ERR_ARG; }
        // the geometry (plm_plan.h), then the arrays it asks for
        knobs = PlmKnobs::from_env();
        PlmShape shape;
        shape.N = N; shape.L = L; shape.q = q; shape.elemBytes = (int)sizeof(T); shape.halo = halo; shape.chunkArg = chunk_; shape.warmArg = warm_;
        shape.carryMode = carry_mode; shape.stripWorld = sWorld; shape.stripRank = sRank; shape.strips = strips;
        plan = plm_make_plan(shape, knobs, PlmKernelShapes{{logits_seq_per_wg(5), logits_seq_per_wg(21), logits_seq_per_wg(kPairQ)},
                                                           {logits_jt(5), logits_jt(21), logits_jt(kPairQ)}});
        const int Lq = L * q, JT = plan.JT;
        const size_t npairs = (size_t)L * (L - 1) / 2;

        freeall();
        lbfgs_alloc = false;
        o = decltype(o)();

        DCA_TRY(dalloc(&dx, plan.P + kVecPad)); DCA_TRY(dalloc(&dg, plan.P + kVecPad));
        DCA_TRY(dalloc(&dWt, (size_t)plan.Wrows * plan.Cs));
        DCA_TRY(dalloc(&dSR, (size_t)N * plan.Cs));                  // S: logit sums
        DCA_TRY(dalloc(&dR, (size_t)(N + kNC) * plan.Cs));           // R = w (p - delta); + kNC zero rows: the scatter kernel's last tile reads past row N-1
        HIP_TRY(hipMemsetAsync(dR, 0, (size_t)(N + kNC) * plan.Cs * sizeof(T), ctx->stream));    // pad columns and halo rows stay zero
        DCA_TRY(dalloc(&dG, plan.num_slabs() * plan.slab_elems()));
        DCA_TRY(dalloc(&dw, N));
        DCA_TRY(dalloc(&dXL, (size_t)ceil_div(plan.gUnits, JT) * JT * plan.Npad));
        DCA_TRY(dalloc(&dXT2, (size_t)plan.gUnits * plan.NT));
        DCA_TRY(dalloc(&dPairs, npairs));
        DCA_TRY(dalloc(&dFxPart, 2 * (size_t)plan.nFxPart));                       // (hi, lo) pairs
        DCA_TRY(dalloc(&dRegPart, 2 * (size_t)(plan.nRegPart + kSumStageBlocks)));      // pairs; + the first-stage sums of the regulariser partials
        DCA_TRY(dalloc(&dVecPart, 2 * 27 * kVecBlocks));      // (hi, lo) pairs
        // with column strips only the owned pairs' (and the window's field blocks') partials are written: the others must read as zero
        HIP_TRY(hipMemsetAsync(dRegPart, 0, 2 * (size_t)(plan.nRegPart + kSumStageBlocks) * sizeof(double), ctx->stream));
        HIP_TRY(hipMemsetAsync(dFxPart, 0, 2 * (size_t)plan.nFxPart * sizeof(double), ctx->stream));
        if (sizeof(T) == 8) {
            DCA_TRY(dalloc(&dColPart, 2 * (size_t)kColSumRowBlocks * Lq));
            if (q == 5) DCA_TRY(dalloc(&dColChunk, 2 * (size_t)plan.numScanChunks * Lq));      // the softmax kernel's per-chunk column sums
            DCA_TRY(dalloc(&dColSum, (size_t)Lq));
        }
        if (strips) { DCA_TRY(dalloc(&dGrecv, plan.grecvOff[sWorld])); DCA_TRY(dalloc(&dXsend, plan.xsendOff[sWorld])); DCA_TRY(dalloc(&dXrecv, plan.xrecvOff[sWorld])); }

        HIP_TRY(hipMemsetAsync(dx, 0, (plan.P + kVecPad) * sizeof(T), ctx->stream));
        HIP_TRY(hipMemsetAsync(dg, 0, (plan.P + kVecPad) * sizeof(T), ctx->stream));
        // the exchange scheme (reduce hook, vector-sharding hook, native mode) survives a re-configuration -- a context whose
        // weights changed must be configured again and would otherwise silently fall back to unreduced local sums
        vlo = 0; vn = plan.P; Ppad = plan.P;
        if (strips) {
            native_mode = 4;
            vlo = plan.oLo; vn = plan.oHi - plan.oLo;
        } else if (native_mode == 4) {
            native_mode = 0;
        }
        if (native_mode == 2 || native_mode == 3) {
            if (!ctx->comm) native_mode = 0;
            else DCA_TRY(set_slices(ctx->comm_rank, ctx->comm_world));
        } else if (comm) {
            DCA_TRY(set_slices(comm_rank, comm_world));
        }
        if (native_mode == 1 && !ctx->comm) native_mode = 0;
        HIP_TRY(hipMemsetAsync(dWt, 0, (size_t)plan.Wrows * plan.Cs * sizeof(T), ctx->stream));
        HIP_TRY(hipMemsetAsync(dG, 0, plan.num_slabs() * plan.slab_elems() * sizeof(T), ctx->stream));

        std::vector<PairIJ> hp(npairs);
        {
            size_t k = 0;
            for (int i = 0; i < L - 1; ++i) for (int j = i + 1; j < L; ++j) hp[k++] = PairIJ{(uint16_t)i, (uint16_t)j};
        }
        HIP_TRY(hipMemcpyAsync(dPairs, hp.data(), npairs * sizeof(PairIJ), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));

        // weights in T.  1/count is formed in T exactly as the reference does
        // (1.f/count, plmdca_numerics.cpp:669) when the counts are known.
        std::vector<T> hw(N);
        {
            std::vector<double> wd(N);
            HIP_TRY(hipMemcpy(wd.data(), ctx->dWd, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
            if (ctx->have_counts) {
                std::vector<uint32_t> cnt(N);
                HIP_TRY(hipMemcpy(cnt.data(), ctx->dCounts, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost));
                for (int n = 0; n < N; ++n) hw[n] = (T)1 / (T)cnt[n];
            } else {
                for (int n = 0; n < N; ++n) hw[n] = (T)wd[n];
            }
        }
        HIP_TRY(hipMemcpy(dw, hw.data(), (size_t)N * sizeof(T), hipMemcpyHostToDevice));

        if (plan.pairs) {
            hipLaunchKernelGGL(plm_build_pair_states_kernel, dim3(ceil_div(plan.Npad, 256), ceil_div(plan.gUnits, JT) * JT), dim3(256), 0,
                               ctx->stream, ctx->dX, dXL, N, plan.Npad, L, Ls, 0, 0x2000u);
            hipLaunchKernelGGL(plm_build_pair_states_kernel, dim3(ceil_div(plan.NT, 256), plan.gUnits), dim3(256), 0, ctx->stream,
                               ctx->dX, dXT2, N, plan.NT, L, Ls, halo, 0x9000u);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        } else {
            hipLaunchKernelGGL(plm_build_logit_states_kernel, dim3(ceil_div(plan.Npad, 256), ceil_div(L, JT) * JT), dim3(256), 0,
                               ctx->stream, ctx->dX, dXL, N, plan.Npad, L, Ls);
            hipLaunchKernelGGL(plm_build_states_kernel, dim3(ceil_div(plan.NT, 256), L), dim3(256), 0, ctx->stream,
                               ctx->dX, dXT2, N, L, Ls, halo, plan.NT);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        configured = true;
        return DCA_OK;
    }

    int configure_strips(double lh, double lJ, int cmode, int chunk_, int warm_) override
    {
        if (!ctx->comm) { dca_set_error("column strips need a communicator: dca_comm_init first"); return DCA_ERR_STATE; }
        if (o.begun && !o.finished) { dca_set_error("the decomposition cannot change during an optimisation"); return DCA_ERR_STATE; }
        // the caller's hooks go only if the new decomposition stands: a failed call leaves them as they were (the engine
        // itself is then unconfigured -- configure() says so -- and must be configured again either way)
        const auto hook0 = hook; const auto hookUser0 = hook_user; const auto comm0 = comm; const auto commUser0 = comm_user;
        const int commRank0 = comm_rank, commWorld0 = comm_world;
        hook = nullptr; hook_user = nullptr; comm = nullptr; comm_user = nullptr; comm_rank = comm_world = 0;
        stripRequested = true;
        const int rc = configure(lh, lJ, cmode, chunk_, warm_, 0, 1);
        stripRequested = false;
        if (rc != DCA_OK) { hook = hook0; hook_user = hookUser0; comm = comm0; comm_user = commUser0; comm_rank = commRank0; comm_world = commWorld0; strips = false; }
        return rc;
    }

    // PlmDCA::initFieldsAndCouplings (plmdca_numerics.cpp:207-249) in T, host side
    // (L*q values from an N*L pass; not worth a kernel).
    int init_x() override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        std::vector<T> hw(N);
        HIP_TRY(hipMemcpy(hw.data(), dw, (size_t)N * sizeof(T), hipMemcpyDeviceToHost));
        T meff = 0;
        for (int n = 0; n < N; ++n) meff += hw[n];
        std::vector<T> h((size_t)L * q, (T)0);
        const uint8_t* X = dca_host_msa(ctx);
        if (!X) return DCA_ERR_HIP;
        for (int n = 0; n < N; ++n)
            for (int i = 0; i < L; ++i) h[(size_t)i * q + X[(size_t)n * L + i]] += hw[n];
        for (int i = 0; i < L; ++i) {
            T* hi = h.data() + (size_t)i * q;
            for (int a = 0; a < q; ++a) hi[a] /= meff;
            for (int a = 0; a < q; ++a) hi[a] = std::log(hi[a] * meff + (T)1);
            T s = 0;
            for (int a = 0; a < q; ++a) s += hi[a];
            const T av = s / (T)q;
            for (int a = 0; a < q; ++a) hi[a] -= av;
        }
        o.trial_ready = false;
        HIP_TRY(hipMemsetAsync(dx, 0, plan.P * sizeof(T), ctx->stream));
        HIP_TRY(hipMemcpyAsync(dx, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DCA_OK;
    }

    template <typename U> int upload(const U* src, T* dst)
    {
        std::vector<T> tmp(plan.P);
        for (size_t i = 0; i < plan.P; ++i) tmp[i] = (T)src[i];
        HIP_TRY(hipMemcpy(dst, tmp.data(), plan.P * sizeof(T), hipMemcpyHostToDevice));
        return DCA_OK;
    }
    template <typename U> int download(const T* src, U* dst)
    {
        std::vector<T> tmp(plan.P);
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(tmp.data(), src, plan.P * sizeof(T), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < plan.P; ++i) dst[i] = (U)tmp[i];
        return DCA_OK;
    }
    int set_x(const void* x, int dtype) override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        o.trial_ready = false;
        if (dtype == DCA_F32) return upload(static_cast<const float*>(x), dx);
        if (dtype == DCA_F64) return upload(static_cast<const double*>(x), dx);
        return DCA_ERR_ARG;
    }
    int get_x(void* x, int dtype) override
    {
        if (!configured) return DCA_ERR_STATE;
        if (native_mode == 4 && !stripEmulate) DCA_TRY(strip_allgather(dx));       // collective, like get_g: every rank calls it
        if (dtype == DCA_F32) return download(dx, static_cast<float*>(x));
        if (dtype == DCA_F64) return download(dx, static_cast<double*>(x));
        return DCA_ERR_ARG;
    }
    int get_g(void* g, int dtype) override
    {
        if (!configured) return DCA_ERR_STATE;
        DCA_TRY(gather_vector(dg));
        if (dtype == DCA_F32) return download(dg, static_cast<float*>(g));
        if (dtype == DCA_F64) return download(dg, static_cast<double*>(g));
        return DCA_ERR_ARG;
    }

    // w_ready: W already holds the table of dx (the fused step pass wrote it with the trial point)
    template <int Q> int launch_eval(bool w_ready)
    {
        hipStream_t st = ctx->stream;
        const size_t npairs = (size_t)L * (L - 1) / 2;
        if (!w_ready) {
            ScopedKernelClock kc(ctx, "plm_expand");
            hipLaunchKernelGGL(plm_expand_kernel<T>, dim3((unsigned)npairs), dim3(256), (size_t)q * q * sizeof(T), st,
                               dx, dWt, dPairs, L, q, plan.Cs, plan.cS0, plan.cS1);
        }
        DCA_ROUND_STAGE(1, dWt, (size_t)plan.Wrows * plan.Cs);
        {
            const int numCT = plan.numCT;
            auto launch = [&](auto kern, int QL) -> int {          // QL: the kernel's alphabet (kPairQ: gUnits site pairs)
                const int numNB = plan.Npad / logits_seq_per_wg(QL);
                const int blocks = numCT * numNB;
                const size_t lds = (size_t)2 * 128 * 512 + (size_t)logits_waves(QL) * 256;   // two tiles + prefetch scratch
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                ScopedKernelClock kc(ctx, "plm_logits");
                hipLaunchKernelGGL(kern, dim3(blocks), dim3(logits_waves(QL) * 64), lds, st, dWt, dXL, dSR, N, plan.Npad, plan.gUnits, plan.Cs, numCT, numNB);
                return DCA_OK;
            };
            bool done = false;
            if constexpr (Q == 5 && sizeof(T) == 4) {
                if (plan.pairs) {
                    if (plan.pairJT == 11) DCA_TRY(launch(plm_logits_kernel<T, kPairQ, 11>, kPairQ));
                    else if (plan.pairJT == 10) DCA_TRY(launch(plm_logits_kernel<T, kPairQ, 10>, kPairQ));
                    else DCA_TRY(launch(plm_logits_kernel<T, kPairQ>, kPairQ));
                    done = true;
                }
            }
            if (!done) DCA_TRY(launch(plm_logits_kernel<T, Q>, Q));
        }
        DCA_ROUND_STAGE(2, dSR, (size_t)N * plan.Cs);
        {
            dim3 grid(ceil_div(plan.Lloc, 64), ceil_div(plan.numScanChunks, 4));
            ScopedKernelClock kc(ctx, "plm_softmax");
            constexpr int softNP = (64 * Q * (int)sizeof(T) + 1023) / 1024;
            const size_t softLds = (size_t)4 * 2 * softNP * 1024;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(plm_softmax_kernel<T, Q>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)softLds));
            // the window's sites: their fields, their alignment column, their columns of S / R
            hipLaunchKernelGGL((plm_softmax_kernel<T, Q>), grid, dim3(256), softLds, st, dSR, dR, dx + (size_t)plan.cS0 * q, ctx->dX + plan.cS0, dw, dFxPart,
                               N, plan.Lloc, Ls, plan.Cs, halo, plan.chunk, plan.warm, carry_mode != DCA_CARRY_EXACT ? 1 : 0, plan.numScanChunks, dColChunk);
        }
        DCA_ROUND_STAGE(4, dR, (size_t)N * plan.Cs);
        {
            const size_t lds = (size_t)2 * kNC * kRowBytes;
            const ScatterStage& sc = plan.scatter;         // one launch, or two when the left-over strips are not merged (plm_plan.h)
            auto launch = [&](auto kern) -> int {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                ScopedKernelClock kc(ctx, "plm_scatter");
                for (int i = 0; i < sc.numLaunches; ++i) {
                    const ScatterLaunch& a = sc.launch[i];
                    hipLaunchKernelGGL(kern, dim3(a.gridX, a.gridY), dim3(sc.threads), lds, st, dR, dXT2, dG,
                                       a.N, a.L, a.Cs, a.halo, a.numChunks, a.NT, a.ctBase, a.numPairs, a.splitX, a.numJG, a.chunksPerSplit, a.slabElems, a.blockChunks,
                                       a.firstBlocksX, a.ctBase2, a.numPairs2, a.splitX2, a.chunksPerSplit2);
                }
                if (sc.sumRemCols)
                    hipLaunchKernelGGL(plm_sum_slabs_cols_kernel<T>, dim3(sc.colsGrid), dim3(256), 0, st, dG,
                                       plan.slab_elems(), plan.Cs, sc.col0, sc.ncols, sc.colRows, sc.colSplit, sc.colZero);
                return DCA_OK;
            };
            if constexpr (sizeof(T) == 8) {
                if (plan.scatWaves == 8) DCA_TRY(launch(plm_scatter_kernel<T, Q, 2, 8>));
                else if (plan.scatWaves == 4) DCA_TRY(launch(plm_scatter_kernel<T, Q, 2, 4>));
                else DCA_TRY(launch(plm_scatter_kernel<T, Q, 2, 16>));
            } else if constexpr (Q == 5) {
                if (plan.pairs) DCA_TRY(launch(plm_scatter_kernel<T, kPairQ, 2, 16>));
                else DCA_TRY(launch(plm_scatter_kernel<T, Q, 2, 16>));
            } else {
                DCA_TRY(launch(plm_scatter_kernel<T, Q, 2, 16>));
            }
        }
        DCA_ROUND_STAGE(8, dG, plan.num_slabs() * plan.slab_elems());
        {
            ScopedKernelClock kc(ctx, "plm_fold");
            const int LqLoc = plan.Lloc * q;
            int foldSlabs = plan.scatSplit;
            if (plan.scatSplit > 2 || (strips && plan.scatSplit > 1)) {     // more than two slabs: one streaming pass is cheaper than strided reads in the fold (and rows that travel are sent summed)
                hipLaunchKernelGGL(plm_sum_slabs_kernel<T>, dim3(2048), dim3(256), 0, st, dG, plan.slab_elems(), plan.scatSplit);
                foldSlabs = 1;
            }
            if (dColSum) {
                if (dColChunk)
                    hipLaunchKernelGGL(plm_colsum_chunks_kernel, dim3(ceil_div(LqLoc, 256), kColSumRowBlocks), dim3(256), 0, st, dColChunk, plan.numScanChunks, LqLoc, dColPart);
                else
                    hipLaunchKernelGGL(plm_colsum_parts_kernel<T>, dim3(ceil_div(LqLoc, 64), kColSumRowBlocks), dim3(256), 0, st, dR, N, plan.Cs, LqLoc, dColPart);
                hipLaunchKernelGGL(plm_colsum_final_kernel, dim3(ceil_div(LqLoc, 256)), dim3(256), 0, st, dColPart, kColSumRowBlocks, LqLoc, dColSum);
            }
            // one GPU: the field fold's few workgroups ride behind the pair fold's in ONE launch (same threads, same sums; a launch
            // boundary and a 5 - 11 us kernel less per evaluation); with strips the gradient-table rows travel in between
            const int nOwned = plan.pairEnd - plan.pairBegin;
            const bool mergeFields = knobs.foldMerge != 0 && !strips && nOwned > 0;
            if (!mergeFields)
            hipLaunchKernelGGL(plm_fold_fields_kernel<T>, dim3(ceil_div(LqLoc, 256)), dim3(256), 0, st, dx + (size_t)plan.cS0 * q, dG, dg + (size_t)plan.cS0 * q,
                               dRegPart + 2 * npairs, LqLoc, q, plan.Cs, (T)lambda_h, add_reg, plan.slab_elems(), foldSlabs, dColSum);
            StripMap sm;
            sm.rank = sRank; sm.world = sWorld; sm.s0 = plan.cS0; sm.s1 = plan.cS1;
            for (int r = 0; r <= sWorld; ++r) sm.site0[r] = plan.siteB[r];
            for (int r = 0; r < sWorld; ++r) { sm.recv[r] = strips && r > sRank ? dGrecv + plan.grecvOff[r] : nullptr; sm.recvCs[r] = strips ? strip_cs(r) : 0; }
            if (strips && !stripEmulate) DCA_TRY(exchange_g());
            const size_t lds = (size_t)kFoldWaves * ((q * q + 3) / 4 * 4) * sizeof(T);
            if (nOwned > 0) {
                const int pairBlocks = ceil_div(nOwned, kFoldWaves);
                FoldFieldsArgs<T> ff{dx + (size_t)plan.cS0 * q, dg + (size_t)plan.cS0 * q, dRegPart + 2 * npairs, LqLoc, (T)lambda_h, dColSum, mergeFields ? pairBlocks : -1};
                hipLaunchKernelGGL(plm_fold_pairs_kernel<T>, dim3((unsigned)(pairBlocks + (mergeFields ? ceil_div(LqLoc, 256) : 0))), dim3(64 * kFoldWaves), lds, st, dx, dG, dg, dPairs,
                                   dRegPart, L, q, plan.Cs, (T)lambda_J, add_reg, plan.slab_elems(), foldSlabs, plan.pairBegin, plan.pairEnd, sm, ff);
            }
        }
        DCA_ROUND_STAGE(16, dg, plan.P);
        // fx = regulariser + data term  -> ctx->dScal[0]
        // (one partial per site pair: summed in two stages, a single workgroup needs 28 us for the 125 000 of config D)
        // (the optimiser on one GPU sums fx inside the two launches of its dot products: eval_scalars)
        fxPending = deferFx;
        if (!deferFx) {
            hipLaunchKernelGGL(dd_sum_chunks_kernel, dim3(kSumStageBlocks), dim3(256), 0, st, dRegPart, plan.nRegPart, dRegPart + 2 * (size_t)plan.nRegPart);
            hipLaunchKernelGGL(dd_sum_final_kernel, dim3(1), dim3(1024), 0, st, dRegPart + 2 * (size_t)plan.nRegPart, kSumStageBlocks, dFxPart, plan.nFxPart, ctx->dScal);
        }
        HIP_TRY(hipGetLastError());
        return DCA_OK;
    }

    // leaves fx in ctx->dScal[0] (device); no host sync unless a reduce hook is set
    // defer_fx: the caller is eval_scalars' (one GPU, no hook: nothing reads fx before the dot products are formed)
    int evaluate_async(bool defer_fx = false, bool w_ready = false)
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        deferFx = defer_fx && knobs.fuseFx != 0 && native_mode == 0 && !hook && !comm && !stripEmulate;
        int rc = (q == 21) ? launch_eval<21>(w_ready) : launch_eval<5>(w_ready);
        if (rc != DCA_OK) return rc;
        o.evals += 1;
        if (native_mode == 4) {
            // column strips: both exchanges happened inside launch_eval; fx is summed with the caller's scalars
        } else if (comm || native_mode == 2 || native_mode == 3) {
            // sharded vectors: sum the shards' gradients, keep this rank's slice; fx is summed with the
            // scalars of the caller (eval_scalars / gradient)
            DCA_TRY(do_comm(DCA_COMM_REDUCE_SCATTER, dg, Ppad, (int)sizeof(T) * 8, "reduce-scatter"));
        } else if (native_mode == 1) {
            DCA_TRY(dca_comm_native_reduce(ctx, dg, plan.P, (int)sizeof(T) * 8, ctx->dScal));      // on the stream: no host round trip
        } else if (hook) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (hook(hook_user, dg, plan.P, (int)sizeof(T) * 8, ctx->dScal) != 0) {
                dca_set_error("reduce hook failed");
                return DCA_ERR_ARG;
            }
        }
        return DCA_OK;
    }

    // sum `count` device doubles ctx->dScal[first..] over the ranks (no-op when vectors are not sharded)
    // one collective of the sharded optimiser: through the native communicator on the stream (no host round trip),
    // or through the caller's hook (the stream is drained first: the hook works outside it)
    int do_comm(int op, void* buf, size_t count, int dtype, const char* what)
    {
        if (native_mode >= 2) return dca_comm_native(ctx, op, buf, count, dtype, native_mode == 3);      // mode 4: only the scalar all-reduce comes here
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (comm(comm_user, op, buf, count, dtype) != 0) { dca_set_error("comm hook failed (%s)", what); return DCA_ERR_ARG; }
        return DCA_OK;
    }
    int reduce_scalars(int first, int count)
    {
        if ((!comm && native_mode < 2) || stripEmulate) return DCA_OK;
        return do_comm(DCA_COMM_ALL_REDUCE, ctx->dScal + first, (size_t)count, DCA_F64, "all-reduce");
    }
    // make a P-vector whose slices are valid on their owners valid everywhere
    int gather_vector(T* v)
    {
        if (!comm && native_mode < 2) return DCA_OK;
        if (native_mode == 4) return stripEmulate ? DCA_OK : strip_allgather(v);
        return do_comm(DCA_COMM_ALL_GATHER, v, Ppad, (int)sizeof(T) * 8, "all-gather");
    }
    // after a step: every rank needs x where its evaluation reads it
    int publish_x()
    {
        if (native_mode == 4) return stripEmulate ? DCA_OK : exchange_x();
        return gather_vector(dx);
    }

    // ---------------- column-strip decomposition: the two exchanges of an evaluation and the all-gather of the API calls
    // (grouped point-to-point transfers on the context's stream; no reference counterpart)
    // A, before expand: the parameters a rank's columns need but another rank owns -- the pairs (j, i) with j on a LOWER
    // rank travel up, packed densely; the fields of its sites come from rank 0.
    int exchange_x()
    {
        const int dt = (int)sizeof(T) * 8;
        const size_t q2 = (size_t)q * q;
        for (int r = sRank + 1; r < sWorld; ++r) {
            const int ni = plan.siteB[r + 1] - plan.siteB[r];
            hipLaunchKernelGGL((strip_pairs_copy_kernel<T, true>), dim3((unsigned)(plan.Lloc * ni)), dim3(64), 0, ctx->stream, dx, dXsend + plan.xsendOff[r], L, q, plan.cS0, plan.cS1, plan.siteB[r], plan.siteB[r + 1]);
        }
        DCA_TRY(dca_comm_p2p_begin(ctx));
        int rc = DCA_OK;
        if (sRank == 0) { for (int r = 1; r < sWorld && rc == DCA_OK; ++r) rc = dca_comm_p2p_send(ctx, dx + (size_t)plan.siteB[r] * q, (size_t)(plan.siteB[r + 1] - plan.siteB[r]) * q, dt, r); }
        else rc = dca_comm_p2p_recv(ctx, dx + (size_t)plan.cS0 * q, (size_t)plan.Lloc * q, dt, 0);
        for (int r = sRank + 1; r < sWorld && rc == DCA_OK; ++r) rc = dca_comm_p2p_send(ctx, dXsend + plan.xsendOff[r], (size_t)plan.Lloc * (plan.siteB[r + 1] - plan.siteB[r]) * q2, dt, r);
        for (int r = 0; r < sRank && rc == DCA_OK; ++r) rc = dca_comm_p2p_recv(ctx, dXrecv + plan.xrecvOff[r], (size_t)(plan.siteB[r + 1] - plan.siteB[r]) * plan.Lloc * q2, dt, r);
        const int rc2 = dca_comm_p2p_end(ctx);
        if (rc != DCA_OK) return rc;
        DCA_TRY(rc2);
        for (int r = 0; r < sRank; ++r) {
            const int nj = plan.siteB[r + 1] - plan.siteB[r];
            hipLaunchKernelGGL((strip_pairs_copy_kernel<T, false>), dim3((unsigned)(nj * plan.Lloc)), dim3(64), 0, ctx->stream, dx, dXrecv + plan.xrecvOff[r], L, q, plan.siteB[r], plan.siteB[r + 1], plan.cS0, plan.cS1);
        }
        HIP_TRY(hipGetLastError());
        return DCA_OK;
    }
    // B, between scatter and fold: the rows of G that belong to the sites of a LOWER rank travel down (whole rows of this
    // rank's window: one contiguous block per peer), the field gradients of this rank's sites go to rank 0.
    int exchange_g()
    {
        const int dt = (int)sizeof(T) * 8;
        DCA_TRY(dca_comm_p2p_begin(ctx));
        int rc = DCA_OK;
        for (int r = 0; r < sRank && rc == DCA_OK; ++r)
            rc = dca_comm_p2p_send(ctx, dG + (size_t)plan.siteB[r] * q * plan.Cs, (size_t)(plan.siteB[r + 1] - plan.siteB[r]) * q * plan.Cs, dt, r);
        for (int r = sRank + 1; r < sWorld && rc == DCA_OK; ++r)
            rc = dca_comm_p2p_recv(ctx, dGrecv + plan.grecvOff[r], (size_t)plan.Lloc * q * strip_cs(r), dt, r);
        if (rc == DCA_OK) {
            if (sRank > 0) rc = dca_comm_p2p_send(ctx, dg + (size_t)plan.cS0 * q, (size_t)plan.Lloc * q, dt, 0);
            else for (int r = 1; r < sWorld && rc == DCA_OK; ++r) rc = dca_comm_p2p_recv(ctx, dg + (size_t)plan.siteB[r] * q, (size_t)(plan.siteB[r + 1] - plan.siteB[r]) * q, dt, r);
        }
        const int rc2 = dca_comm_p2p_end(ctx);
        if (rc != DCA_OK) return rc;
        return rc2;
    }
    // every rank's owned range of a P-vector to every other rank, in place (get_x / get_g / scores: not on the hot path)
    int strip_allgather(T* v)
    {
        const int dt = (int)sizeof(T) * 8;
        DCA_TRY(dca_comm_p2p_begin(ctx));
        int rc = DCA_OK;
        for (int k = 1; k < sWorld && rc == DCA_OK; ++k) {
            const int to = (sRank + k) % sWorld, from = (sRank - k + sWorld) % sWorld;
            rc = dca_comm_p2p_send(ctx, v + plan.oLo, plan.oHi - plan.oLo, dt, to);
            if (rc == DCA_OK) rc = dca_comm_p2p_recv(ctx, v + owned_lo(from), owned_hi(from) - owned_lo(from), dt, from);
        }
        const int rc2 = dca_comm_p2p_end(ctx);
        if (rc != DCA_OK) return rc;
        return rc2;
    }
    int bm_source(void** x) override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        if (o.begun && !o.finished) { dca_set_error("an L-BFGS run is in progress: dca_plm_lbfgs_end first"); return DCA_ERR_STATE; }
        if (strips || native_mode == 4) { dca_set_error("Boltzmann learning runs on one GPU: configured for column strips"); return DCA_ERR_STATE; }
        if (comm || hook || native_mode != 0) {
            dca_set_error("Boltzmann learning runs on one GPU: vector sharding, a reduce / comm hook or a native-comm mode is set");
            return DCA_ERR_STATE;
        }
        *x = dx;
        return DCA_OK;
    }
    int transform_source(void** x) override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        if (strips || native_mode == 4 || comm || hook || native_mode != 0) {
            dca_set_error("the gauge transformation runs on one GPU: column strips, vector sharding, a reduce / comm hook or a native-comm mode is set");
            return DCA_ERR_STATE;
        }
        o.trial_ready = false;
        *x = dx;
        return DCA_OK;
    }
    // the current x for energy.hip, pll.hip, sample.hip, sample_conditional.hip, ascent.hip and ais.hip; an L-BFGS run in progress is
    // allowed.  Column strips gather x first, as scores() does; one_gpu_only (AIS, conditional sampling, ascent) refuses them instead
    int potts_source(PottsSource* out, bool one_gpu_only) override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        if (one_gpu_only) {
            if (strips || native_mode == 4) { dca_set_error("AIS, conditional sampling and the ascent run on one GPU: configured for column strips"); return DCA_ERR_STATE; }
            if (comm || hook || native_mode != 0) {
                dca_set_error("AIS, conditional sampling and the ascent run on one GPU: vector sharding, a reduce / comm hook or a native-comm mode is set");
                return DCA_ERR_STATE;
            }
        } else if (native_mode == 4 && !stripEmulate) {
            DCA_TRY(strip_allgather(dx));
        }
        *out = PottsSource{dx, 0, (int)sizeof(T) * 8, nullptr, L, q, 0};
        return DCA_OK;
    }
    int set_vector_sharding(int rank, int world, dca_comm_hook h, void* user) override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        if (o.begun && !o.finished) { dca_set_error("vector sharding cannot change during an optimisation"); return DCA_ERR_STATE; }
        if (strips) { dca_set_error("configured for column strips: dca_plm_configure again first"); return DCA_ERR_STATE; }
        if (native_mode >= 2) native_mode = 0;
        if (!h || world < 1) { vlo = 0; vn = plan.P; Ppad = plan.P; comm = nullptr; comm_user = nullptr; comm_rank = comm_world = 0; return DCA_OK; }
        DCA_TRY(set_slices(rank, world));
        comm = h; comm_user = user; comm_rank = rank; comm_world = world;
        return DCA_OK;
    }
    int set_slices(int rank, int world)
    {
        if (rank < 0 || rank >= world || world > 64) { dca_set_error("bad rank / world"); return DCA_ERR_ARG; }
        const size_t slice = (plan.P + (size_t)world * 4 - 1) / ((size_t)world * 4) * 4;    // multiple of 4 elements: 16-byte aligned slices
        if (slice * world > plan.P + kVecPad) { dca_set_error("world too large for the vector padding"); return DCA_ERR_ARG; }
        Ppad = slice * world;
        vlo = slice * rank;
        vn = vlo >= plan.P ? 0 : std::min(slice, plan.P - vlo);
        return DCA_OK;
    }
    bool configured_for_comm() const override { return configured; }
    int set_native_comm(int mode) override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        if (o.begun && !o.finished) { dca_set_error("the exchange scheme cannot change during an optimisation"); return DCA_ERR_STATE; }
        if (mode != 0 && !ctx->comm) { dca_set_error("no communicator: dca_comm_init first"); return DCA_ERR_STATE; }
        if (mode == 4) { dca_set_error("the column-strip decomposition is set up by dca_plm_configure_strips"); return DCA_ERR_ARG; }
        if (mode < 0 || mode > 3) return DCA_ERR_ARG;
        if (strips) {       // the arrays are cut for a column window: another scheme (or none) needs a new configuration
            if (mode != 0) { dca_set_error("configured for column strips: dca_plm_configure again first"); return DCA_ERR_STATE; }
            configured = false; strips = false; native_mode = 0; o = decltype(o)();
            return DCA_OK;
        }
        if (mode >= 2) DCA_TRY(set_slices(ctx->comm_rank, ctx->comm_world));      // validate before anything is dropped
        else { vlo = 0; vn = plan.P; Ppad = plan.P; }
        comm = nullptr; comm_user = nullptr; comm_rank = comm_world = 0;
        if (mode != 0) { hook = nullptr; hook_user = nullptr; }                   // the native exchange replaces the caller's hook
        native_mode = mode;
        return DCA_OK;
    }

    int read_scalars(int n)
    {
        HIP_TRY(hipMemcpyAsync(ctx->hScal, ctx->dScal, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DCA_OK;
    }

    int gradient(double* fx_out) override
    {
        o.trial_ready = false;              // W becomes the table of the accepted point
        DCA_TRY(evaluate_async());
        DCA_TRY(reduce_scalars(0, 1));
        DCA_TRY(gather_vector(dg));
        DCA_TRY(read_scalars(1));
        if (fx_out) *fx_out = ctx->hScal[0];
        return DCA_OK;
    }

    // ---------------- vector helpers
    void v_neg(T* d, const T* g) { hipLaunchKernelGGL(vec_neg_kernel<T>, dim3(kVecBlocks), dim3(kVecThreads), 0, ctx->stream, d + vlo, g + vlo, vn); }
    void v_step(T* x, const T* xp, double stp, const T* d) { hipLaunchKernelGGL(vec_step_kernel<T>, dim3(kVecBlocks), dim3(kVecThreads), 0, ctx->stream, x + vlo, xp + vlo, (T)stp, d + vlo, vn); }
    // after an evaluation: fx (slot 0), g.d, x.x, g.g (slots 1..3) in one round trip
    int eval_scalars(double* fx, double* gd, double* xx, double* gg)
    {
        if (fxPending) {
            double* const fxChunks = dRegPart + 2 * (size_t)plan.nRegPart;
            hipLaunchKernelGGL(vec_dot3_fx_kernel<T>, dim3(kVecBlocks + kSumStageBlocks), dim3(kVecThreads), 0, ctx->stream, dg + vlo, dd + vlo, dx + vlo, vn, dVecPart,
                               dRegPart, plan.nRegPart, fxChunks);
            hipLaunchKernelGGL(vec_final_fx_kernel, dim3(3 + 1), dim3(1024), 0, ctx->stream, dVecPart, kVecBlocks, 3, ctx->dScal + 1,
                               fxChunks, kSumStageBlocks, dFxPart, plan.nFxPart, ctx->dScal);
            fxPending = false;
        } else {
            hipLaunchKernelGGL(vec_dot3_kernel<T>, dim3(kVecBlocks), dim3(kVecThreads), 0, ctx->stream, dg + vlo, dd + vlo, dx + vlo, vn, dVecPart);
            hipLaunchKernelGGL(vec_final_kernel, dim3(3), dim3(256), 0, ctx->stream, dVecPart, kVecBlocks, 3, ctx->dScal + 1);
        }
        DCA_TRY(reduce_scalars(0, 4));     // fx (local data term) and the three partial dot products
        DCA_TRY(read_scalars(kSlotDginit + 1));
        *fx = ctx->hScal[0]; *gd = ctx->hScal[1]; *xx = ctx->hScal[2]; *gg = ctx->hScal[3];
        if (o.dginit_on_device) { o.dginit = ctx->hScal[kSlotDginit]; o.dginit_on_device = false; }
        return DCA_OK;
    }

    int lbfgs_begin(int max_iterations, int verbose) override
    {
        if (!configured) { dca_set_error("dca_plm_configure first"); return DCA_ERR_STATE; }
        if (!lbfgs_alloc) {
            DCA_TRY(dalloc(&dxp, plan.P + kVecPad)); DCA_TRY(dalloc(&dgp, plan.P + kVecPad)); DCA_TRY(dalloc(&dd, plan.P + kVecPad));
            for (int i = 0; i < 5; ++i) { DCA_TRY(dalloc(&dS[i], plan.P + kVecPad)); DCA_TRY(dalloc(&dY[i], plan.P + kVecPad)); }
            HIP_TRY(hipMemsetAsync(dxp, 0, (plan.P + kVecPad) * sizeof(T), ctx->stream));
            HIP_TRY(hipMemsetAsync(dgp, 0, (plan.P + kVecPad) * sizeof(T), ctx->stream));
            HIP_TRY(hipMemsetAsync(dd, 0, (plan.P + kVecPad) * sizeof(T), ctx->stream));
            lbfgs_alloc = true;
        }
        for (int i = 0; i < 5; ++i) {   // unused history slots take part in the Gram kernel as zeros
            HIP_TRY(hipMemsetAsync(dS[i], 0, (plan.P + kVecPad) * sizeof(T), ctx->stream));
            HIP_TRY(hipMemsetAsync(dY[i], 0, (plan.P + kVecPad) * sizeof(T), ctx->stream));
        }
        if (!dLb) HIP_TRY(dca_dev_malloc(reinterpret_cast<void**>(&dLb), sizeof(LbfgsDev)));
        HIP_TRY(hipMemsetAsync(dLb, 0, sizeof(LbfgsDev), ctx->stream));
        o = decltype(o)();
        o.max_iterations = max_iterations;
        o.verbose = verbose;
        auto t0 = std::chrono::steady_clock::now();
        DCA_TRY(evaluate_async(true));
        v_neg(dd, dg);
        double fx, gd, xx, gg;
        DCA_TRY(eval_scalars(&fx, &gd, &xx, &gg));
        o.fx = fx;
        o.xnorm = std::sqrt(xx); o.gnorm = std::sqrt(gg);
        const double xn = std::max(o.xnorm, 1.0);
        o.begun = true;
        if (o.gnorm / xn <= 1e-3) { o.status = LB_ALREADY_MINIMIZED; o.finished = true; }
        o.step = 1.0 / std::sqrt(gg);      // 1/|d| with d = -g   (lbfgs.cpp:459)
        o.dginit = -gg;
        o.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return DCA_OK;
    }

    // More-Thuente line search (more_thuente.h) on device vectors.  Returns the number of evaluations (>0) or a libLBFGS
    // error code; *rc_hip carries runtime failures.
    int line_search(double* stp, double* f, double* xx, double* gg, int* rc_hip)
    {
        const MtParams params{1e-4, 0.9, 1e-16, 1e-20, 1e20, 5};     // plmdcaBackend.cpp:68-75 over lbfgs.cpp:116-121
        // g.d of the direction: known on the host, or still on its way from the device's two-loop recursion -- then
        // eval_scalars brings it into o.dginit with the scalars of the first evaluation
        const bool deferred = o.dginit_on_device;
        bool first = true;
        const int ls = mt_line_search(params, stp, f, &o.dginit, deferred, [&](double t, double* ft, double* dgt) {
            // the fused step pass left this trial point in dx and its table in W: only the first trial, only at step 1 exactly
            const bool ready = o.trial_ready && first && t == 1.0 && fused_step_ok();
            o.trial_ready = false; first = false;
            if (!ready) {
                v_step(dx, dxp, t, dd);
                DCA_ROUND_STAGE(32, dx, plan.P);
            }
            DCA_TRY(publish_x());                 // sharded vectors: every rank needs the x its evaluation reads
            DCA_TRY(evaluate_async(true, ready));
            return eval_scalars(ft, dgt, xx, gg);
        }, rc_hip);
        if (deferred && ls == LB_INCREASEGRADIENT) o.evals -= 1;     // the reference returns before evaluating (lbfgs.cpp:858-861); the caller restores x, g
        return ls;
    }

    void lbfgs_end() override { o = decltype(o)(); }
    // The fused step pass is for the plain one-GPU path: everything else keeps the three kernels.
    bool fused_step_ok() const
    {
#ifdef DCA_ROUND_ABLATE
        if (round_stage_mask()) return false;
#endif
        return knobs.fuseStep != 0 && native_mode == 0 && !hook && !comm && !strips && !stripEmulate && vlo == 0 && vn == plan.P &&
               plan.cS0 == 0 && plan.cS1 == L;
    }
    // d, the trial point x + 1 * d (into dxp: the next iteration's swap makes it dx) and its table W
    template <int Q> void launch_fused_step(const VecPtrs5& ptrs)
    {
        const int numJC = ceil_div(L, fused_step_jc(Q)), pairBlocks = ceil_div(L, fused_step_ti(Q, (int)sizeof(T))) * numJC;
        const size_t lds = (size_t)fused_step_ti(Q, (int)sizeof(T)) * fused_step_jc(Q) * Q * Q * sizeof(T);
        hipLaunchKernelGGL((lbfgs_dir_trial_expand_kernel<T, Q>), dim3((unsigned)(ceil_div(pairBlocks, 64) * 64 + ceil_div(L * Q, kFusedStepThreads))), dim3(kFusedStepThreads), lds,
                           ctx->stream, dd, dxp, dWt, dx, dg, ptrs, &dLb->cf, L, plan.Cs, numJC, pairBlocks);
    }
    int lbfgs_iterate(int iterations, dca_plm_stats* st) override
    {
        if (!o.begun) { dca_set_error("dca_plm_lbfgs_begin first"); return DCA_ERR_STATE; }
        auto t0 = std::chrono::steady_clock::now();
        constexpr int M = 5;
        for (int it = 0; it < iterations && !o.finished; ++it) {
            // the current point becomes (xp, gp) by swapping buffers: the line search writes
            // x = xp + step*d and the evaluation writes g into the other pair (lbfgs.cpp:465-466)
            std::swap(dx, dxp);
            std::swap(dg, dgp);
            double xx = 0, gg = 0;
            int rc = 0;
            const int ls = line_search(&o.step, &o.fx, &xx, &gg, &rc);
            if (rc) return rc;
            if (ls < 0) {   // revert to the previous point (lbfgs.cpp:478-484)
                std::swap(dx, dxp);
                std::swap(dg, dgp);
                o.trial_ready = false;
                o.status = ls; o.finished = true;
                break;
            }
            o.xnorm = std::sqrt(xx); o.gnorm = std::sqrt(gg);
            o.iters = o.k;
            o.last_step = o.step;
            if (o.verbose) {
                fprintf(stderr, "Iteration %d:\n", o.k);
                fprintf(stderr, "fx = %f, xnorm = %f, gnorm = %f, step = %f\n\n", o.fx, o.xnorm, o.gnorm, o.step);
            }
            const double xn = std::max(o.xnorm, 1.0);
            if (o.gnorm / xn <= 1e-3) { o.status = 0; o.finished = true; break; }
            if (o.max_iterations != 0 && o.max_iterations < o.k + 1) { o.status = LB_MAXIMUMITERATION; o.finished = true; break; }

            // s, y of the accepted step and every dot product the direction needs, in one kernel and ONE
            // round trip for the scalars: dScal[1..2] = y.s, y.y;  dScal[3..27] = the 25 Gram entries
            const int e = o.end;              // slot of the newest pair
            VecPtrs5 ptrs;
            for (int i = 0; i < M; ++i) { ptrs.s[i] = dS[i] + vlo; ptrs.y[i] = dY[i] + vlo; }
            {
                ScopedKernelClock kc(ctx, "lbfgs_vec");
                auto gram = [&](auto slot) {
                    hipLaunchKernelGGL((vec_diff_gram_kernel<T, decltype(slot)::value>), dim3(kVecBlocks), dim3(kVecThreads), 0, ctx->stream, ptrs, dS[e] + vlo, dY[e] + vlo,
                                       dx + vlo, dxp + vlo, dg + vlo, dgp + vlo, vn, dVecPart);
                };
                switch (e) {
                case 0: gram(std::integral_constant<int, 0>()); break;
                case 1: gram(std::integral_constant<int, 1>()); break;
                case 2: gram(std::integral_constant<int, 2>()); break;
                case 3: gram(std::integral_constant<int, 3>()); break;
                default: gram(std::integral_constant<int, 4>()); break;
                }
                hipLaunchKernelGGL(vec_final_kernel, dim3(27), dim3(256), 0, ctx->stream, dVecPart, kVecBlocks, 27, ctx->dScal + 1);
            }
            DCA_TRY(reduce_scalars(1, 27));
            const int bound = (M <= o.k) ? M : o.k;
            ++o.k;
            o.end = (o.end + 1) % M;
            {
                // two-loop recursion on the device (no host round trip), then d = cf.g g + sum cf.s_k s_k + cf.y_k y_k
                ScopedKernelClock kc(ctx, "lbfgs_vec");
                hipLaunchKernelGGL(lbfgs_two_loop_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->dScal, dLb, e, o.end, bound, gg);
                if (fused_step_ok()) {
                    if (q == 21) launch_fused_step<21>(ptrs); else launch_fused_step<5>(ptrs);
                    o.trial_ready = true;
                } else {
                    hipLaunchKernelGGL(vec_compose_kernel<T>, dim3(kVecBlocks), dim3(kVecThreads), 0, ctx->stream, dd + vlo, dg + vlo, ptrs, &dLb->cf, vn);
                    DCA_ROUND_STAGE(64, dd, plan.P);
                }
                o.dginit_on_device = true;
            }
            o.step = 1.0;
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        o.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (st) {
            st->status = o.status; st->iterations = o.iters; st->evaluations = o.evals; st->finished = o.finished ? 1 : 0;
            st->fx = o.fx; st->xnorm = o.xnorm; st->gnorm = o.gnorm; st->step = o.iters ? o.last_step : o.step; st->seconds = o.seconds;
        }
        return DCA_OK;
    }

    int scores(int apc, double* out) override
    {
        if (!configured) return DCA_ERR_STATE;
        if (native_mode == 4 && !stripEmulate) DCA_TRY(strip_allgather(dx));
        const size_t npairs = (size_t)L * (L - 1) / 2;
        double* dOut = nullptr;
        HIP_TRY(dca_dev_malloc(reinterpret_cast<void**>(&dOut), npairs * sizeof(double)));
        int rc = dca_fn_scores(ctx, dx, 0, (int)sizeof(T) * 8, L, q, 0, apc, dOut);
        if (rc == DCA_OK) {
            // ctx->stream is non-blocking: the null-stream copy below does not wait for it
            hipError_t e = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess) e = hipMemcpy(out, dOut, npairs * sizeof(double), hipMemcpyDeviceToHost);
            if (e != hipSuccess) { dca_set_error("copy scores: %s", hipGetErrorString(e)); rc = DCA_ERR_HIP; }
        }
        dca_dev_free(dOut);
        return rc;
    }
    // (q-1)x(q-1) blocks of the current x for selected pairs (compute_params, plmdca.py:345-434)
    int pair_couplings(const int* pairs, int npairs, int shift, double* out) override
    {
        if (!configured) return DCA_ERR_STATE;
        if (native_mode == 4 && !stripEmulate) DCA_TRY(strip_allgather(dx));
        return dca_pair_blocks(ctx, dx, 0, (int)sizeof(T) * 8, L, q, 0, pairs, npairs, shift, out);
    }

    // DI of the current x (plmdca.py:683-790); reg_fi: host, L*q regularised single-site frequencies
    int di_scores(const double* reg_fi, int apc, double* out) override
    {
        if (!configured) return DCA_ERR_STATE;
        if (native_mode == 4 && !stripEmulate) DCA_TRY(strip_allgather(dx));
        const size_t npairs = (size_t)L * (L - 1) / 2;
        double *dOut = nullptr, *dFi = nullptr;
        HIP_TRY(dca_dev_malloc(reinterpret_cast<void**>(&dOut), npairs * sizeof(double)));
        if (dca_dev_malloc(reinterpret_cast<void**>(&dFi), (size_t)L * q * sizeof(double)) != hipSuccess) { dca_dev_free(dOut); return DCA_ERR_NOMEM; }
        int rc = DCA_OK;
        if (hipMemcpy(dFi, reg_fi, (size_t)L * q * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = DCA_ERR_HIP;
        if (rc == DCA_OK) rc = dca_di_scores(ctx, dx, 0, (int)sizeof(T) * 8, dFi, L, q, 0, apc, dOut);
        if (rc == DCA_OK) {
            hipError_t e = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess) e = hipMemcpy(out, dOut, npairs * sizeof(double), hipMemcpyDeviceToHost);
            if (e != hipSuccess) { dca_set_error("copy DI scores: %s", hipGetErrorString(e)); rc = DCA_ERR_HIP; }
        }
        dca_dev_free(dOut); dca_dev_free(dFi);
        return rc;
    }
};

}  // namespace

PlmEngineBase* dca_make_plm_engine(dca_ctx* ctx)
{
    if (ctx->precision == DCA_F64) return new PlmEngine<double>(ctx);
    return new PlmEngine<float>(ctx);
}
