// Launch geometry of the kernels that read the fitted Potts model as a sequence model: the pair tiles of the energies
// (energy.hip), the chunking of the site conditionals (site_conditionals.h: pll.hip, ardca.hip), the chunking of the Gibbs sweep
// (sample.hip, ais.hip; sample_conditional.hip at its F free sites), the pair tiles of the bmDCA statistics (boltzmann.hip,
// bm_pairs.h) and the chunks of the decimation's selection (decimation.hip), each from (L, q, element size) alone.
// Host code only, no HIP header: a host compiler builds it, and tests/potts_plan_driver.cpp prints it for
// tests/test_potts_audit_host.py, which holds the audit's case table to these numbers.  Included from dca_internal.h.
#pragma once

#include <algorithm>
#include <cstddef>

static inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- energy.hip: energy_pairs_kernel<S, TS>
constexpr int kESeqBlock = 4096;                   // sequences per workgroup = kEThreads * kESeqPerThread (energy.hip asserts it)
constexpr size_t kETileBudget = 72 * 1024;         // LDS per tile: two workgroups per CU (160 KiB), one loads while one gathers
constexpr int kETargetGroups = 128;                // tile groups (slabs) for large L
constexpr int kEChunk = 16 * kESeqBlock;           // query sequences per pass (bounds the slabs: G x 65536 doubles)

struct EnergyGeom { int TS, nb, ntiles, tpg, G; };

inline EnergyGeom energy_geometry(int L, int q, size_t elem)
{
    static const int kSizes[] = {24, 16, 12, 8, 6, 4, 3};
    EnergyGeom g{};
    for (int ts : kSizes)
        if ((size_t)ts * ts * q * q * elem <= kETileBudget) { g.TS = ts; break; }
    g.nb = ceil_div(L, g.TS);
    g.ntiles = g.nb * (g.nb + 1) / 2;
    g.tpg = ceil_div(g.ntiles, kETargetGroups);
    g.G = ceil_div(g.ntiles, g.tpg);
    return g;
}

// dynamic LDS of the pair kernel: one tile, TS x TS pairs of q x q values
inline size_t energy_lds(int TS, int q, size_t elem) { return (size_t)TS * TS * q * q * elem; }

// ---- site_conditionals.h: site_conditional_body<S, QM, Policy>
constexpr int kSiteThreads = 256;                           // 4 waves
constexpr int kSitePerLane = 2;                             // queries per lane
constexpr int kSiteSeqBlock = kSiteThreads * kSitePerLane;  // queries per workgroup: one staging of a site's blocks serves 512
constexpr int kSiteMaxCJ = 16;                              // blocks per chunk at most (bounds the code chunk to 8 KiB)
constexpr size_t kSiteChunkBudget = 16 * 1024;              // LDS per block chunk buffer (two of them)

// accumulators per query: the state count rounded up to a multiple of the 16-byte LDS reads
inline int qm_of(int q) { return q <= 8 ? 8 : q <= 24 ? 24 : 32; }

// Blocks per chunk: a chunk buffer holds CJ blocks of up to QM x QM values within kSiteChunkBudget (at most kSiteMaxCJ)
template <typename S, int QM>
constexpr int chunk_blocks() { return (int)(kSiteChunkBudget / (QM * QM * sizeof(S))) < kSiteMaxCJ ? (int)(kSiteChunkBudget / (QM * QM * sizeof(S))) : kSiteMaxCJ; }

// block elements per thread (q * q <= 256 * KPB)
template <int QM>
constexpr int site_kpb() { return (QM * QM + kSiteThreads - 1) / kSiteThreads; }

// 16-byte code pieces per thread (the chunk's codes: CJ x 512 bytes)
template <typename S, int QM>
constexpr int site_cpt() { return (chunk_blocks<S, QM>() * kSiteSeqBlock / 16 + kSiteThreads - 1) / kSiteThreads; }

// dynamic LDS of a site kernel: two chunk buffers (CJ blocks of q x QM values of S each), then two code buffers (CJ x 512 bytes)
template <typename S, int QM>
size_t site_lds(int q)
{
    constexpr int CJ = chunk_blocks<S, QM>();
    return round_up(2 * (size_t)CJ * q * QM * sizeof(S), 16) + 2 * (size_t)CJ * kSiteSeqBlock;
}

// the same per run-time (q, element size), for the driver
struct SitePlan { int QM, CJ, KPB, CPT; size_t lds; };

template <typename S, int QM>
SitePlan site_plan_of(int q) { return {QM, chunk_blocks<S, QM>(), site_kpb<QM>(), site_cpt<S, QM>(), site_lds<S, QM>(q)}; }

template <typename S>
SitePlan site_plan_t(int q)
{
    switch (qm_of(q)) {
    case 8: return site_plan_of<S, 8>(q);
    case 24: return site_plan_of<S, 24>(q);
    default: return site_plan_of<S, 32>(q);
    }
}

inline SitePlan site_plan(int q, size_t elem) { return elem == 4 ? site_plan_t<float>(q) : site_plan_t<double>(q); }

// ---- sample.hip: gibbs_sweep_kernel<S, QM, RES, R, MODE>
constexpr int kSThreads = 256;                    // 4 waves, 64 chains
constexpr int kSChains = 64;
constexpr int kSResidentL = 512;                  // chain codes in LDS up to 32 KiB
constexpr size_t kSChunkBudget = 40 * 1024;       // LDS per J chunk buffer (two of them)

// chunk elements per thread
constexpr int sample_regs(size_t elem) { return elem == 4 ? 32 : 16; }

struct SampleGeom { int QM, CJ; bool res; size_t lds; };

inline SampleGeom sample_geometry(int L, int q, size_t elem)
{
    SampleGeom g{};
    g.QM = qm_of(q);
    const size_t blkBytes = (size_t)q * g.QM * elem;
    const int R = sample_regs(elem);
    int cj = std::min((int)(kSThreads * R / (q * q)), (int)(kSChunkBudget / blkBytes));
    g.CJ = std::max(4, cj / 4 * 4);
    g.res = L <= kSResidentL;
    g.lds = round_up(2 * (size_t)g.CJ * blkBytes, 16) + (size_t)g.QM * kSChains * sizeof(double) + (g.res ? (size_t)L * kSChains : 0);
    return g;
}

// ---- sample_conditional.hip: cond_sweep_kernel<S, QM, RES, R> over F free sites and cond_fields_kernel<S, QM, R>
constexpr int kCFieldChains = 256;                // chains per workgroup of the field pass (lane = chain)
constexpr size_t kCFieldBudget = (size_t)1 << 30; // the field buffer of one block of chains (F x q doubles per chain)

// chunk elements per thread of the field pass: half the sweep's, every lane holds all QM accumulators there
constexpr int cond_field_regs(size_t elem) { return sample_regs(elem) / 2; }

// The sweep's geometry is the plain sweep's at F sites (the chunks run over the free positions, the free sites' codes sit in LDS up
// to kSResidentL of them, and then the site list follows them there: F ints); the field pass
// stages chunks of CJF = CJ / 2 blocks through two buffers and keeps nothing else in LDS.
struct CondSampleGeom { int QM, CJ, CJF; bool res; size_t lds, ldsFields; };

inline CondSampleGeom cond_sample_geometry(int F, int q, size_t elem)
{
    const SampleGeom s = sample_geometry(F, q, elem);
    const int cjf = s.CJ / 2;
    return {s.QM, s.CJ, cjf, s.res, s.lds + (s.res ? (size_t)F * sizeof(int) : 0), round_up(2 * (size_t)cjf * q * s.QM * elem, 16)};
}

// ---- boltzmann.hip: bm_pairs_kernel<S, TB, UPDATE>
constexpr int kBmThreads = 256;
constexpr int kBmSums = 6;                 // slab: max |d|, sum Cd, sum Cm, sum Cd^2, sum Cm^2, sum Cd Cm

// site-pair tile edge: the tile's histogram (TB^2 q^2 uint32) stays within 64 KiB
inline int bm_tile(int q) { return q <= 8 ? 16 : q <= 24 ? 4 : 2; }

// dynamic LDS of the pair kernel (the histogram) and its static LDS (the reduction buffer)
inline size_t bm_lds(int TB, int q) { return (size_t)TB * TB * q * q * sizeof(unsigned); }
constexpr size_t kBmStaticLds = (size_t)kBmSums * kBmThreads * sizeof(double);

// ---- decimation.hip: dec_hist_kernel, dec_count_kernel / dec_apply_kernel, gauge_pairs_kernel
constexpr int kDecThreads = 256;
constexpr int kDecChunk = 16 * kDecThreads;        // consecutive elements per workgroup of the count and apply passes
constexpr int kDecHistBlocks = 2048;               // grid of a histogram pass at most (grid-stride; 8 workgroups per CU)
constexpr int kGaugeThreads = 256;
constexpr int kGaugeMaxQ = 32;                     // states per site the gauge kernels hold in static LDS (dca_set_msa's limit)

inline size_t dec_chunks(size_t n) { return (n + kDecChunk - 1) / kDecChunk; }
inline int dec_hist_blocks(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>((n + kDecThreads - 1) / kDecThreads, kDecHistBlocks)); }
