// Replica-exchange (parallel-tempering) Gibbs sampling of a fitted Potts model on a ladder betas[0] < ... < betas[R-1]
// (dca_plm_sample_tempered, dca_mf_sample_tempered).  M ladders of R walkers each; walker r of ladder m is
// row m * R + r of the state and Philox chain (first_ladder + m) * R + r.  A walker keeps its codes for ever and carries a level;
// it sweeps under betas[level]:
//   sweep g     sample.hip's sweep kernel, kSweepTempered instantiation: the plain sweep with chain c's own beta read from a
//               device array (betaChain[c]; 0 for the padding chains), one launch for all walkers (tag "sample");
//   round rho   after sweep g when (g + 1) mod I == 0, rho = (g + 1) / I - 1: E of every walker (energy.hip's pair kernels on the
//               chain state, then pt_energy_kernel, which forms E exactly as energy_finish_kernel does; tag "pt_energy"), then
//               pt_swap_kernel (tag "pt_swap"): per ladder and k = rho (mod 2), k + 1 < R, with a the walker at level k and b the
//               one at level k + 1, d = (betas[k+1] - betas[k]) * (E_a - E_b) (both differences first, one multiply),
//               U = philox_uniform(seed, first_ladder + m, rho, k, 5), accept iff d >= 0 || U < exp(d); accepting exchanges the
//               two walkers' levels (and so their betaChain entries).
// pt_swap_kernel runs one thread per (ladder, slot p): the slot owns the levels k = (rho mod 2) + 2 p and k + 1 (slot 0 of an odd
// round also level 0), so no two threads touch the same level, walker or trace element; it writes the round's row of the energy
// trace for its levels before it decides.  The only atomics are the integer attempt / accept counters, whose sums do not depend
// on the order.  Nothing leaves the device between rounds except the trace, which is flushed in blocks of rounds.
// The device scratch stays within kPtScratchBudget by running blocks of ladders one after another (a ladder depends on nothing
// but itself, so the split does not show; DCA_PT_PASS caps the ladders of a block) and by flushing the trace buffer
// (kPtTraceBudget of it; DCA_PT_TRACE_ROUNDS caps its rounds).
#include "dca_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

constexpr int kPtStride = 128;                          // chain stride of the state: the energy kernels' multiple
constexpr int kPtMaxWalkers = 1 << 24;
constexpr size_t kPtScratchBudget = (size_t)1 << 30;    // all device buffers of a call
constexpr size_t kPtTraceBudget = (size_t)1 << 28;      // ... of which the trace buffer
constexpr uint32_t kPtTag = 5;

// E[c] of walker c < n; E as energy_finish_kernel forms it from the fields and the slabs
template <typename S>
__global__ __launch_bounds__(256)
void pt_energy_kernel(const PottsView<S> pv, const uint8_t* __restrict__ QT, int n, int NqS, const double* __restrict__ slabs, int G,
                      double* __restrict__ E)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double e = 0.0;
    for (int i = 0; i < pv.L; ++i) e += pv.field(i, QT[(size_t)i * NqS + c]);
    for (int g = 0; g < G; ++g) e += slabs[(size_t)g * NqS + c];
    E[c] = e;
}

// Exchange round `round` of the ladders ladder0 .. ladder0 + M - 1.  Thread t = m * P + p, P = R / 2 + 1 slots per ladder.
// level[m * R + r]: the level of walker r; walkerAt[m * R + k]: the walker at level k; betaChain[m * R + r] = betas[level].
// traceRow (or NULL): M x R doubles, E of the walker at level k before the exchange.  attempts / accepts: R - 1 counters.
__global__ __launch_bounds__(256)
void pt_swap_kernel(int M, int R, const double* __restrict__ betas, const double* __restrict__ E, int* __restrict__ level,
                    int* __restrict__ walkerAt, double* __restrict__ betaChain, uint64_t seed, uint64_t ladder0, uint64_t round,
                    double* __restrict__ traceRow, unsigned long long* __restrict__ attempts, unsigned long long* __restrict__ accepts)
{
    const int P = R / 2 + 1;
    const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
    if (t >= (size_t)M * P) return;
    const int m = (int)(t / P), p = (int)(t % P);
    const int par = (int)(round & 1);
    const size_t base = (size_t)m * R;
    int* wa = walkerAt + base;
    if (par == 1 && p == 0 && traceRow) traceRow[base] = E[base + wa[0]];
    const int k = par + 2 * p;
    if (k >= R) return;
    const int a = wa[k];
    const double ea = E[base + a];
    if (traceRow) traceRow[base + k] = ea;
    if (k + 1 >= R) return;
    const int b = wa[k + 1];
    const double eb = E[base + b];
    if (traceRow) traceRow[base + k + 1] = eb;
    const double db = betas[k + 1] - betas[k], de = ea - eb;
    const double d = db * de;
    bool accept = d >= 0.0;
    if (!accept) accept = philox_uniform(seed, ladder0 + (uint64_t)m, round, k, kPtTag) < exp(d);
    atomicAdd(&attempts[k], 1ull);
    if (!accept) return;
    atomicAdd(&accepts[k], 1ull);
    wa[k] = b; wa[k + 1] = a;
    level[base + a] = k + 1; level[base + b] = k;
    betaChain[base + a] = betas[k + 1]; betaChain[base + b] = betas[k];
}

// positive value of an environment variable, or 0
long env_count(const char* name)
{
    const char* v = getenv(name);
    return v && atol(v) > 0 ? atol(v) : 0;
}

// E of the block's walkers into dE (under "pt_energy")
hipError_t energy_pass(dca_ctx* ctx, const PottsSource& ps, const DcaChains& ch, double* dSlabs, int G, double* dE)
{
    ScopedKernelClock kc(ctx, "pt_energy");
    HIP_PASS(dca_energy_pairs_device(ctx, ps, ch.dState, ch.n, ch.nS, dSlabs));
    with_source_type(ps, [&](auto pv) {
        hipLaunchKernelGGL(pt_energy_kernel, dim3(ceil_div(ch.n, 256)), dim3(256), 0, ctx->stream, pv, (const uint8_t*)ch.dState.get(), ch.n,
                           ch.nS, (const double*)dSlabs, G, dE);
    });
    return hipGetLastError();
}

}  // namespace

int dca_potts_sample_tempered(dca_ctx* ctx, const PottsSource& ps, const dca_pt_args* args, uint8_t* out, int32_t* levels_out,
                              double* energies_out, uint64_t* attempts_out, uint64_t* accepts_out, double* energy_trace_out,
                              int* rounds_out)
{
    static const char* who = "sample_tempered";
    const int L = ps.L, q = ps.q;
    if (!args) { dca_set_error("%s: args is NULL", who); return DCA_ERR_ARG; }
    const int M = args->ladders, R = args->levels, sweeps = args->sweeps, I = args->swap_interval;
    if (M < 0 || R < 1 || sweeps < 0 || I < 0 || (long long)M * R > kPtMaxWalkers || args->first_sweep > UINT64_MAX - (uint64_t)sweeps) {
        dca_set_error("%s: bad counts (ladders %d, levels %d, sweeps %d, swap_interval %d; at most 2^24 walkers)", who, M, R, sweeps, I);
        return DCA_ERR_ARG;
    }
    if (!args->betas) { dca_set_error("%s: betas is NULL", who); return DCA_ERR_ARG; }
    for (int k = 0; k < R; ++k) {
        const double b = args->betas[k];
        if (!std::isfinite(b) || b < 0.0 || (k > 0 && !(b > args->betas[k - 1]))) {
            dca_set_error("%s: betas must be finite, >= 0 and strictly increasing (betas[%d] = %g)", who, k, b);
            return DCA_ERR_ARG;
        }
    }
    if (M > 0 && (!out || !levels_out)) { dca_set_error("%s: out or levels_out is NULL", who); return DCA_ERR_ARG; }
    const uint64_t fs = args->first_sweep, seed = args->seed;
    const int rounds = I > 0 ? (int)((fs + (uint64_t)sweeps) / (uint64_t)I - fs / (uint64_t)I) : 0;
    if (rounds_out) *rounds_out = rounds;
    for (int k = 0; k + 1 < R; ++k) {
        if (attempts_out) attempts_out[k] = 0;
        if (accepts_out) accepts_out[k] = 0;
    }
    if (M == 0) return DCA_OK;
    const size_t n = (size_t)M * R;
    if (args->initial_levels) {
        std::vector<char> seen((size_t)R);
        for (int m = 0; m < M; ++m) {
            std::fill(seen.begin(), seen.end(), 0);
            for (int r = 0; r < R; ++r) {
                const int32_t l = args->initial_levels[(size_t)m * R + r];
                if (l < 0 || l >= R || seen[l]) {
                    dca_set_error("%s: initial_levels of ladder %d are not a permutation of 0 .. %d (walker %d: %d)", who, m, R - 1, r, (int)l);
                    return DCA_ERR_ARG;
                }
                seen[l] = 1;
            }
        }
    }
    if (args->initial) DCA_TRY(dca_check_codes(args->initial, n * L, q, "sample_tempered: initial "));

    // ladders per block and trace rounds per flush
    const int G = dca_energy_slab_count(ps);
    const bool trace = energy_trace_out && rounds > 0;
    const size_t perWalker = 2 * (size_t)L + (size_t)G * sizeof(double) + 2 * sizeof(double) + 2 * sizeof(int);
    const size_t forWalkers = kPtScratchBudget - kPtTraceBudget;      // per walker: the state, its row copy, slabs, E, beta, level, walkerAt
    size_t Mb = std::max<size_t>(1, std::min<size_t>((size_t)M, (forWalkers / perWalker - std::min(forWalkers / perWalker, (size_t)kPtStride)) / R));
    if (env_count("DCA_PT_PASS")) Mb = std::min(Mb, (size_t)env_count("DCA_PT_PASS"));
    size_t Fb = trace ? std::max<size_t>(1, std::min<size_t>((size_t)rounds, kPtTraceBudget / (Mb * R * sizeof(double)))) : 0;
    if (trace && env_count("DCA_PT_TRACE_ROUNDS")) Fb = std::min(Fb, (size_t)env_count("DCA_PT_TRACE_ROUNDS"));
    const size_t nbMax = Mb * R, nSMax = round_up(nbMax, kPtStride);

    DevBuf<double> dBetas, dBetaChain, dSlabs, dE, dTrace;
    DevBuf<int> dLevel, dWalkerAt;
    DevBuf<unsigned long long> dCounts;
    HIP_TRY_AS_NOMEM(dBetas.alloc((size_t)R, false), who);
    HIP_TRY_AS_NOMEM(dBetaChain.alloc(nSMax, false), who);
    HIP_TRY_AS_NOMEM(dLevel.alloc(nSMax, false), who);
    HIP_TRY_AS_NOMEM(dWalkerAt.alloc(nbMax, false), who);
    HIP_TRY_AS_NOMEM(dCounts.alloc(2 * (size_t)R, false), who);
    if (rounds > 0 || energies_out) {
        HIP_TRY_AS_NOMEM(dSlabs.alloc((size_t)G * nSMax, false), who);
        HIP_TRY_AS_NOMEM(dE.alloc(nSMax, false), who);
    }
    if (trace) HIP_TRY_AS_NOMEM(dTrace.alloc(Fb * nbMax, false), who);
    unsigned long long* dAttempts = dCounts.get();
    unsigned long long* dAccepts = dCounts.get() + R;
    HIP_TRY_AS(hipMemcpyAsync(dBetas, args->betas, (size_t)R * sizeof(double), hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS(hipMemsetAsync(dCounts, 0, 2 * (size_t)R * sizeof(unsigned long long), ctx->stream), who);

    std::vector<int> hLevel(nSMax), hWalkerAt(nbMax);
    std::vector<double> hBetaChain(nSMax);
    for (size_t m0 = 0; m0 < (size_t)M; m0 += Mb) {
        const int mb = (int)std::min(Mb, (size_t)M - m0), nb = mb * R;
        const uint64_t ladder0 = args->first_ladder + (uint64_t)m0, first_chain = ladder0 * (uint64_t)R;
        DcaChains ch;
        DCA_TRY(dca_chains_start(ctx, &ch, nb, L, q, seed, first_chain, args->initial ? args->initial + m0 * R * L : nullptr, kPtStride));
        std::fill(hLevel.begin(), hLevel.end(), 0);
        std::fill(hBetaChain.begin(), hBetaChain.end(), 0.0);          // the padding chains sweep under beta = 0
        for (int c = 0; c < nb; ++c) {
            const int l = args->initial_levels ? args->initial_levels[m0 * R + c] : c % R;
            hLevel[c] = l;
            hWalkerAt[(size_t)(c / R) * R + l] = c % R;
            hBetaChain[c] = args->betas[l];
        }
        HIP_TRY_AS(hipMemcpyAsync(dLevel, hLevel.data(), (size_t)ch.nS * sizeof(int), hipMemcpyHostToDevice, ctx->stream), who);
        HIP_TRY_AS(hipMemcpyAsync(dWalkerAt, hWalkerAt.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, ctx->stream), who);
        HIP_TRY_AS(hipMemcpyAsync(dBetaChain, hBetaChain.data(), (size_t)ch.nS * sizeof(double), hipMemcpyHostToDevice, ctx->stream), who);

        // rows 0 .. held - 1 of the trace buffer are the rounds flushed .. flushed + held - 1 of this call
        size_t flushed = 0, held = 0;
        auto flush = [&]() -> hipError_t {
            if (!held) return hipSuccess;
            HIP_PASS(hipMemcpy2DAsync(energy_trace_out + (flushed * M + m0) * R, n * sizeof(double), dTrace, (size_t)nb * sizeof(double),
                                      (size_t)nb * sizeof(double), held, hipMemcpyDeviceToHost, ctx->stream));
            flushed += held;
            held = 0;
            return hipStreamSynchronize(ctx->stream);
        };
        uint64_t g = fs;                                               // the global number of the next sweep
        for (int left = sweeps; left > 0;) {
            const int run = I > 0 ? (int)std::min<uint64_t>((uint64_t)left, (uint64_t)I - g % (uint64_t)I) : left;
            DCA_TRY(dca_chains_sweeps(ctx, ch, ps, run, seed, first_chain, g, 0.0, nullptr, 0.0, dBetaChain));
            g += (uint64_t)run;
            left -= run;
            if (I == 0 || g % (uint64_t)I != 0) continue;
            const uint64_t rho = g / (uint64_t)I - 1;
            HIP_TRY_AS(energy_pass(ctx, ps, ch, dSlabs, G, dE), who);
            {
                ScopedKernelClock kc(ctx, "pt_swap");
                const size_t threads = (size_t)mb * (R / 2 + 1);
                hipLaunchKernelGGL(pt_swap_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, mb, R,
                                   (const double*)dBetas.get(), (const double*)dE.get(), dLevel.get(), dWalkerAt.get(), dBetaChain.get(), seed,
                                   ladder0, rho, trace ? dTrace.get() + held * nb : (double*)nullptr, dAttempts, dAccepts);
                HIP_TRY_AS(hipGetLastError(), who);
            }
            if (trace && ++held == Fb) HIP_TRY_AS(flush(), who);
        }
        if (trace) HIP_TRY_AS(flush(), who);
        HIP_TRY_AS(hipMemcpyAsync(levels_out + m0 * R, dLevel, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream), who);
        if (energies_out) {
            HIP_TRY_AS(energy_pass(ctx, ps, ch, dSlabs, G, dE), who);
            HIP_TRY_AS(hipMemcpyAsync(energies_out + m0 * R, dE, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), who);
        }
        DCA_TRY(dca_chains_read(ctx, ch, out + m0 * R * L));
    }
    if (R > 1 && attempts_out)
        HIP_TRY_AS(hipMemcpyAsync(attempts_out, dAttempts, (size_t)(R - 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), who);
    if (R > 1 && accepts_out)
        HIP_TRY_AS(hipMemcpyAsync(accepts_out, dAccepts, (size_t)(R - 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}
