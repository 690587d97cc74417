// Launch geometry of the plmDCA engine (plm_engine.hip) as a pure host function: everything PlmEngine::configure decides
// before it allocates -- the column window, the scan's chunking, the site-pair alphabet and its tile, the padded array shapes,
// the scatter stage's split / left-over strips / float64 canonical geometry -- from (N, L, q, element size, halo, window) and
// the tuning knobs.  Standard C++ only (no HIP, no context, no environment inside plm_make_plan): tests/test_plm_plan_host.py
// compiles it with the host compiler and holds it to recorded decisions.  The float32 gradient's bits depend on this output:
// it fixes the order in which the slabs of G are summed.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "../../include/dca_hip.h"

namespace {

// ---- constants shared by the planner and the kernels (plm_stages.h, lbfgs_kernels.h)
constexpr int kPlanXcds = 8;        // = kNumXcd (dca_internal.h; plm_engine.hip asserts it)
constexpr int kPairQ = 25;          // the site-pair alphabet of q = 5 (plm_stages.h)
constexpr int kNC = 128;            // sequences per scatter tile
constexpr int kRowBytes = 512;      // bytes of one staged row (64 lanes x 8 B)
constexpr int kScatWavesC = 16;
constexpr int kCanonBlock = 16384;  // float64 mode: sequences per block of the canonical summation order (= ORACLE_CANONICAL_BLOCK)
static_assert(kCanonBlock % kNC == 0, "canonical blocks are whole tiles");
constexpr int kColSumRowBlocks = 64;
// first stage for long partial vectors: block b sums its contiguous chunk (fixed tree) into out[b]
constexpr int kSumStageBlocks = 64;
constexpr int kMaxStripRanks = 64;
// vector sharding (dca_plm_set_vector_sharding): collectives run over Ppad = world * slice elements, inside this padding
constexpr size_t kVecPad = 256;

struct PlmShape {
    int N = 0, L = 0, q = 0;
    int elemBytes = 4;                      // 4 | 8
    int halo = 0;
    int chunkArg = 0, warmArg = 0;          // <= 0: the planner chooses
    int carryMode = DCA_CARRY_CHUNKED;
    int stripWorld = 1, stripRank = 0;      // column-strip decomposition: this rank of so many (1, 0 without it)
    bool strips = false;
};

// Tuning / test knobs (README.md, environment variables); -1 = unset.
struct PlmKnobs {
    int scatterRem = -1;        // DCA_SCATTER_REM: 0 never, 1 whenever there are left-over strips
    int scatterSplit = -1;      // DCA_SCATTER_SPLIT: the split of the main launch
    int scatterCanon = -1;      // DCA_SCATTER_CANON: 1 one workgroup, 2 slab per block
    int scatterWaves = -1;      // DCA_SCATTER_WAVES: waves of the one-workgroup geometry
    int plmPairs = -1;          // DCA_PLM_PAIRS: 0 = the per-site blocks for q = 5 in float32
    int scatterMerge = -1;      // DCA_SCATTER_MERGE: 0 = the left-over strips as a launch of their own
    int foldMerge = -1;         // DCA_FOLD_MERGE: 0 = the field fold as a launch of its own
    int fuseFx = -1;            // DCA_PLM_FUSE_FX: 0 = fx summed by its own two kernels
    int fuseStep = -1;          // DCA_PLM_FUSE_STEP: 0 = direction, trial point and expand as their own three kernels
    bool is_set(int v) const { return v != -1; }
    // the only place where the engine reads these nine variables: once per configure
    static PlmKnobs from_env()
    {
        PlmKnobs k;
        auto rd = [](const char* name, int& v) { if (const char* e = getenv(name)) { v = atoi(e); if (v == -1) v = -2; } };
        rd("DCA_SCATTER_REM", k.scatterRem); rd("DCA_SCATTER_SPLIT", k.scatterSplit); rd("DCA_SCATTER_CANON", k.scatterCanon);
        rd("DCA_SCATTER_WAVES", k.scatterWaves); rd("DCA_PLM_PAIRS", k.plmPairs); rd("DCA_SCATTER_MERGE", k.scatterMerge);
        rd("DCA_FOLD_MERGE", k.foldMerge); rd("DCA_PLM_FUSE_FX", k.fuseFx);
        rd("DCA_PLM_FUSE_STEP", k.fuseStep);
        return k;
    }
};

// what the planner has to know of the generated logits blocks (logits_gather_asm.inc), index 0 / 1 / 2 = q 5 / 21 / kPairQ
struct PlmKernelShapes {
    int logitsSeqPerWg[3];      // sequences per workgroup
    int logitsJT[3];            // sites (kPairQ: site pairs) per LDS tile
    static int slot(int q) { return q == 21 ? 1 : q == kPairQ ? 2 : 0; }
};

// One launch of plm_scatter_kernel: the grid and the arguments behind (R, XT2, G), in the kernel's order.
struct ScatterLaunch {
    unsigned gridX = 0, gridY = 1;
    int N = 0, L = 0, Cs = 0, halo = 0, numChunks = 0, NT = 0, ctBase = 0, numPairs = 0, splitX = 1, numJG = 0, chunksPerSplit = 0;
    size_t slabElems = 0;
    int blockChunks = 0;
    int firstBlocksX = 0x7fffffff, ctBase2 = 0, numPairs2 = 0, splitX2 = 1, chunksPerSplit2 = 0;     // no second set of pairs
};
// The scatter stage: one launch, or two when the left-over strips are not merged into the main one, and the sum of the
// left-over strips' slabs (plm_sum_slabs_cols_kernel) behind them.
struct ScatterStage {
    int threads = 0;
    int numLaunches = 0;
    ScatterLaunch launch[2];
    bool sumRemCols = false;                          // left-over strips: slab 0 of their columns = the sum of their slabs
    unsigned colsGrid = 0;
    int col0 = 0, ncols = 0, colRows = 0, colSplit = 0, colZero = 0;
};

struct PlmPlan {
    // column window (the whole alignment unless the column-strip decomposition is on) and the packed parameters this rank owns
    std::vector<int> siteB;                           // site boundaries of the ranks (world + 1)
    int cS0 = 0, cS1 = 0, Lloc = 0;
    size_t oLo = 0, oHi = 0;
    int pairBegin = 0, pairEnd = 0;
    // softmax scan
    int chunk = 128, warm = 40, numScanChunks = 0, numScatChunks = 0;
    // arrays
    size_t P = 0;
    int Cs = 0;                        // row stride (elements) of W, SR, G
    // q = 5 in float32: both gather kernels walk site PAIRS on the 25-state combined alphabet (kPairQ; DCA_PLM_PAIRS=0: the
    // per-site blocks, for comparisons).  gUnits = what the kernels' "L" counts: pairs then, sites otherwise.
    bool pairs = false;
    int gUnits = 0;
    int pairJT = 12;                   // site pairs per LDS tile of the logits kernel: of 12 / 11 / 10 the count that pads gUnits least
    int JT = 0;                        // units per logits tile
    int Wrows = 0, Grows = 0, Npad = 0, NT = 0;
    // scatter
    int scatJW = 2, scatWaves = kScatWavesC;
    int scatSplit = 1, scatChunksPerSplit = 0;
    int scatBlockChunks = 0;           // float64 mode: tiles per canonical block of sequences (0: plain chains)
    bool scatPerBlock = false;         // ... with one workgroup and one slab of G per block
    int scatRemCT = 0, scatRemSplit = 0, scatRemChunksPerSplit = 0;     // left-over strips (numCT % 8) with their own, finer split
    int numCT = 0;                     // 512-byte column strips
    bool scatDealPairs = false;        // the (strip, split) pairs, not the strips, are dealt to the XCDs
    ScatterStage scatter;
    int nFxPart = 0, nRegPart = 0;
    // column strips: per peer, elements; [world] = the totals
    std::vector<size_t> grecvOff, xsendOff, xrecvOff;

    int logits_q(int q) const { return pairs ? kPairQ : q; }
    size_t slab_elems() const { return (size_t)Grows * Cs; }
    int num_slabs() const { return std::max(scatSplit, scatRemSplit); }
};

inline size_t plm_pair_start(int L, int s) { return (size_t)L * (L - 1) / 2 - (size_t)(L - s) * (L - s - 1) / 2; }     // pairs whose first site is < s
inline int plm_strip_cs(const std::vector<int>& siteB, int q, int r) { return (int)(((size_t)(siteB[r + 1] - siteB[r]) * q + 127) / 128 * 128); }
inline size_t plm_owned_lo(const std::vector<int>& siteB, int L, int q, int r) { return r == 0 ? 0 : (size_t)L * q + plm_pair_start(L, siteB[r]) * q * q; }
inline size_t plm_owned_hi(const std::vector<int>& siteB, int L, int q, int r) { return (size_t)L * q + plm_pair_start(L, siteB[r + 1]) * q * q; }

// The scatter stage's launches from the plan.  Three shapes of the (main) launch: (strip, split) pairs dealt to the XCDs; the
// main strips with the split in blockIdx.y; main and left-over strips in one grid (the left-over workgroups behind the main
// ones of every row).
inline ScatterStage plm_scatter_stage(const PlmShape& s, const PlmPlan& p, const PlmKnobs& knobs)
{
    auto ceil_div = [](int a, int b) { return (a + b - 1) / b; };
    const int CW = kRowBytes / s.elemBytes;
    const int numCT = p.numCT;
    const int numJG = ceil_div(p.gUnits, p.scatWaves * p.scatJW);
    const int mainCT = numCT - p.scatRemCT;            // strips of the main launch (all of them without a left-over launch)
    const int remPairs = p.scatRemCT * p.scatRemSplit;
    const bool mergeRem = knobs.scatterMerge != 0 && !p.scatDealPairs;
    ScatterStage st;
    st.threads = p.scatWaves * 64;
    ScatterLaunch base;
    base.N = s.N; base.L = p.gUnits; base.Cs = p.Cs; base.halo = s.halo; base.numChunks = p.numScatChunks; base.NT = p.NT;
    base.ctBase = 0; base.numJG = numJG; base.slabElems = p.slab_elems(); base.blockChunks = p.scatBlockChunks;
    ScatterLaunch m = base;
    if (p.scatDealPairs) {       // E: 6 strips would leave two XCDs idle: deal the (strip, split) pairs to the XCDs instead
        m.gridX = (unsigned)(kPlanXcds * ceil_div(numCT * p.scatSplit, kPlanXcds) * numJG);
        m.numPairs = numCT * p.scatSplit; m.splitX = p.scatSplit; m.chunksPerSplit = p.scatChunksPerSplit;
    } else {
        const int mainX = kPlanXcds * ceil_div(mainCT, kPlanXcds) * numJG;
        m.gridX = (unsigned)mainX; m.gridY = (unsigned)p.scatSplit;
        m.numPairs = mainCT; m.splitX = 1; m.chunksPerSplit = p.scatChunksPerSplit;
        if (p.scatRemCT && mergeRem) {
            m.gridX += (unsigned)(kPlanXcds * ceil_div(remPairs, kPlanXcds) * numJG);
            m.firstBlocksX = mainX; m.ctBase2 = mainCT; m.numPairs2 = remPairs; m.splitX2 = p.scatRemSplit; m.chunksPerSplit2 = p.scatRemChunksPerSplit;
        }
    }
    st.launch[st.numLaunches++] = m;
    if (p.scatRemCT) {
        if (!mergeRem) {
            ScatterLaunch r = base;
            r.gridX = (unsigned)(kPlanXcds * ceil_div(remPairs, kPlanXcds) * numJG);
            r.ctBase = mainCT; r.numPairs = remPairs; r.splitX = p.scatRemSplit; r.chunksPerSplit = p.scatRemChunksPerSplit; r.blockChunks = 0;
            st.launch[st.numLaunches++] = r;
        }
        st.sumRemCols = true;
        st.col0 = mainCT * CW; st.ncols = p.Cs - st.col0; st.colRows = s.L * s.q;
        st.colsGrid = (unsigned)(((size_t)st.colRows * st.ncols + 255) / 256);
        st.colSplit = p.scatRemSplit; st.colZero = p.scatSplit;
    }
    return st;
}

inline PlmPlan plm_make_plan(const PlmShape& s, const PlmKnobs& knobs, const PlmKernelShapes& ks)
{
    auto ceil_div = [](int a, int b) { return (a + b - 1) / b; };
    auto round_up = [](size_t v, size_t m) { return (v + m - 1) / m * m; };
    const int N = s.N, L = s.L, q = s.q, halo = s.halo, sWorld = s.stripWorld, sRank = s.stripRank;
    const size_t elem = (size_t)s.elemBytes;
    PlmPlan p;
    p.siteB.assign(sWorld + 1, 0);
    for (int r = 0; r <= sWorld; ++r) p.siteB[r] = (int)((long long)L * r / sWorld);
    p.cS0 = p.siteB[sRank]; p.cS1 = p.siteB[sRank + 1]; p.Lloc = p.cS1 - p.cS0;
    p.oLo = plm_owned_lo(p.siteB, L, q, sRank); p.oHi = plm_owned_hi(p.siteB, L, q, sRank);
    p.pairBegin = (int)plm_pair_start(L, p.cS0); p.pairEnd = (int)plm_pair_start(L, p.cS1);
    const int Lloc = p.Lloc;

    // scan chunk: 256 sequences (15 % warm-up rows instead of 31 %) when that still leaves at least one
    // chunk-wave per SIMD and the rows are long (q = 21; config D: 1.20 -> 0.99 ms; with q = 5 the chain
    // latency dominates and 128 stays faster), else 128
    p.chunk = s.chunkArg > 0 ? s.chunkArg : ((q >= 16 && (long long)ceil_div(N - halo, 256) * ceil_div(Lloc, 64) >= 1024) ? 256 : 128);
    // small alignments: the scan is a chain of one step per sequence and wave, so shorter chunks (more waves, more
    // warm-up rows of a small array) until there is about one chunk-wave per SIMD: config C 0.30 -> 0.16 ms with 32
    if (s.chunkArg <= 0)
        while (p.chunk > 32 && (long long)ceil_div(N - halo, p.chunk) * ceil_div(Lloc, 64) < 1024) p.chunk /= 2;
    // warm-up steps of the chunk-parallel scan: 2^-40 of start-up error is far below float rounding; the float64 mode is
    // the parity mode and takes 80, with which the chunked scan is BIT-identical to the serial chain (the start-up
    // error has dropped below the last place of every carried probability; 100 iterations at configs D and E end in the
    // same bits, profiles/r04_sensitivity_*.json)
    p.warm = s.warmArg > 0 ? s.warmArg : (elem == 8 ? 80 : 40);
    if (s.carryMode == DCA_CARRY_SERIAL) { p.chunk = N - halo; p.warm = halo; }
    if (s.carryMode == DCA_CARRY_EXACT) p.warm = 0;
    p.numScanChunks = ceil_div(N - halo, p.chunk);
    p.numScatChunks = ceil_div(N - halo, kNC);
    const int numScatChunks = p.numScatChunks;

    p.P = (size_t)L * q + (size_t)L * (L - 1) / 2 * q * q;     // dca_plm_num_params
    const int Lq = L * q;
    const int LqLoc = Lloc * q;
    p.Cs = (int)round_up(LqLoc, 128);
    p.pairs = q == 5 && elem == 4 && knobs.plmPairs != 0;
    p.gUnits = p.pairs ? ceil_div(L, 2) : L;
    p.pairJT = 12;
    if (p.pairs)
        for (int jt : {11, 10})
            if (ceil_div(p.gUnits, jt) * jt < ceil_div(p.gUnits, p.pairJT) * p.pairJT) p.pairJT = jt;      // L = 150: 75 pairs = 7 x 11 (77) rather than 7 x 12 (84)
    const int JT = p.JT = p.pairs ? p.pairJT : ks.logitsJT[PlmKernelShapes::slot(q)];       // units per logits tile
    p.Wrows = ceil_div(p.gUnits, JT) * (p.pairs ? JT * 2 * q : JT * q) + 128;     // + over-read margin of the last LDS-DMA tile
    p.scatJW = 2;     // units per wave of the scatter kernel
    const int JG = kScatWavesC * p.scatJW;
    p.Grows = ceil_div(p.gUnits, JG) * JG * (p.pairs ? 2 * q : q);
    p.Npad = (int)round_up(N, ks.logitsSeqPerWg[PlmKernelShapes::slot(p.logits_q(q))]);
    const int gUnits = p.gUnits, Grows = p.Grows, Cs = p.Cs, scatJW = p.scatJW;
    {
        // Split of the tile range (every split writes its own slab of G) and the left-over launch.  Strips are dealt to
        // the XCDs in sets of eight (plm_scatter_kernel), the numJG site groups of a strip and split run side by side on
        // one XCD's 32 CUs, and a workgroup costs its tiles + about two for prologue and epilogue.  numCT % 8 left-over
        // strips keep that many XCDs busy for whole extra rounds while the others idle (D: 83 strips = 11 rounds on
        // three XCDs, 10 on five), so they may get their own launch with a finer split that spreads them over all XCDs
        // for a fraction of a round.  Every extra slab costs the fold one more pass over G (about `slabUnits` tile
        // times).  Model: cost = rounds x (tiles per workgroup + 2) [+ the same for the left-over launch] + slabs;
        // candidates up to ~2048 workgroups with >= 12 tiles each.  Measured (tools/time_eval.py, DCA_SCATTER_SPLIT /
        // DCA_SCATTER_REM; scatter + fold, ms): D 1 + left-over 7.28 (split 2 without: 7.74), D/8 1.19 (1.34),
        // C 0.376 (0.458 for the best split without a left-over launch), E split 19-32: 0.90 (51: 0.93).
        constexpr int kNumXcd = kPlanXcds;
        const int cw = kRowBytes / (int)elem;
        const int numCT = p.numCT = ceil_div(Cs, cw), numJGs = ceil_div(gUnits, JG);
        const int fullCT = numCT / kNumXcd * kNumXcd, rem = numCT - fullCT;
        const int s0 = std::max(1, std::min({numScatChunks, ceil_div(2048, numCT * numJGs), std::max(1, numScatChunks / 12)}));
        const int cuPerXcd = 256 / kNumXcd;
        auto rounds = [&](long long wgsPerXcd) { return (double)((wgsPerXcd + cuPerXcd - 1) / cuPerXcd); };
        const double slabUnits = (double)Grows * Cs * elem / 4e12 / 4e-6;      // one pass over a slab at ~4 TB/s, in 4 us tile times
        const bool remSet = knobs.is_set(knobs.scatterRem);         // tuning / test knob: 0 never, 1 whenever there are left-over strips
        const bool splitSet = knobs.is_set(knobs.scatterSplit);     // tuning knob: the split of the main launch
        double bestCost = 1e300;
        p.scatSplit = 1; p.scatChunksPerSplit = numScatChunks; p.scatRemCT = p.scatRemSplit = p.scatRemChunksPerSplit = 0;
        // float64 = parity mode: the oracle's order of summation -- per (site, state, column) the sequences in ascending
        // order inside blocks of kCanonBlock, the block sums added in ascending block order (the test oracle's
        // ORACLE_CANONICAL_BLOCK; round 4: one chain over all N) -- so that the gradient does not depend on the launch
        // geometry.  Two geometries give exactly that order: ONE workgroup per (strip, site group) that adds its
        // finished block to the running sum in G and restarts its chains (plm_scatter_kernel, blockChunks), or one
        // workgroup and one slab PER BLOCK, the slabs summed in ascending order by plm_sum_slabs_kernel.  The second
        // fills the chip where strips x site groups do not (config E: 12 x 5 = 60 workgroups, 13 blocks: scatter 4.03 ->
        // 1.39 ms), the first saves the slab traffic where they do (config D: 2656 workgroups, 4 blocks: 14.4 ms against
        // 16.6 + 0.9 in the fold; round 4's single chain 13.3 -- each of the three read-modify-write passes over G stalls
        // the lock-stepped workgroups for 0.35 ms, which is why the blocks are 16384 and not 4096 sequences).  No separate
        // launch for the left-over strips; a test that forces a split or that launch leaves the canonical order.
        const bool canonical = elem == 8 && !splitSet && !remSet;
        p.scatWaves = kScatWavesC;
        p.scatBlockChunks = 0;
        p.scatPerBlock = false;
        if (canonical) {
            p.scatBlockChunks = kCanonBlock / kNC;
            const int nblocks = ceil_div(numScatChunks, p.scatBlockChunks);
            const int we = knobs.scatterWaves;          // tuning knob (one-workgroup geometry)
            const int ge = knobs.scatterCanon;          // tuning / test knob: 1 one workgroup, 2 slab per block
            auto perXcdOf = [&](int waves, int sp) {
                const int njg = ceil_div(gUnits, waves * scatJW);
                return fullCT > 0 ? (long long)ceil_div(numCT, kNumXcd) * njg * sp : (long long)ceil_div(numCT * sp, kNumXcd) * njg;
            };
            // one workgroup: 16 waves, or 8 where that does not fill the chip (twice the workgroups; 4 waves measured slower)
            int wavesA = kScatWavesC;
            if (we == 16 || we == 8 || we == 4) wavesA = we;
            else if ((long long)numCT * ceil_div(gUnits, kScatWavesC * scatJW) < 192) wavesA = 8;
            // (a tile of an 8-wave workgroup takes 0.85 of a 16-wave one's time: E 3.87 against 4.53 ms on one round each;
            // the (strip, block) pairs of the second geometry are dealt to the XCDs one by one, see plm_scatter_stage)
            const double costA = rounds(perXcdOf(wavesA, 1)) * (numScatChunks * (wavesA == 8 ? 0.85 : 1.0) + 2.0 + 0.5 * (nblocks - 1));
            const double costB = rounds((long long)ceil_div(numCT * nblocks, kNumXcd) * numJGs) * (p.scatBlockChunks + 2.0) + (nblocks - 1) * slabUnits;
            p.scatPerBlock = nblocks > 1 && (knobs.is_set(ge) ? ge == 2 : costB < costA);
            if (p.scatPerBlock) { p.scatSplit = nblocks; p.scatChunksPerSplit = p.scatBlockChunks; }
            else p.scatWaves = wavesA;
        }
        for (int sp = 1; sp <= (canonical ? 0 : (splitSet ? numScatChunks : s0)); ++sp) {
            if (splitSet && sp != std::max(1, std::min(numScatChunks, knobs.scatterSplit))) continue;
            const int cps = ceil_div(numScatChunks, sp);
            if (ceil_div(numScatChunks, cps) != sp && !splitSet) continue;               // same as a smaller split
            const int spEff = ceil_div(numScatChunks, cps);
            const double slabs = (spEff - 1) * slabUnits;
            if (!(knobs.scatterRem == 1 && fullCT > 0 && rem > 0)) {
                // fewer than eight strips: the (strip, split) pairs, not the strips, are dealt to the XCDs (plm_scatter_stage)
                const long long perXcd = fullCT > 0 ? (long long)ceil_div(numCT, kNumXcd) * numJGs * spEff
                                                    : (long long)ceil_div(numCT * spEff, kNumXcd) * numJGs;
                const double cost = rounds(perXcd) * (cps + 2.0) + slabs;
                if (cost < bestCost) { bestCost = cost; p.scatSplit = spEff; p.scatChunksPerSplit = cps; p.scatRemCT = p.scatRemSplit = p.scatRemChunksPerSplit = 0; }
            }
            if (fullCT > 0 && rem > 0 && knobs.scatterRem != 0) {
                int sB = std::max(spEff, 256 / (rem * numJGs));
                sB = std::max(1, std::min(sB, std::max(1, numScatChunks / 12)));
                const int cpsB = ceil_div(numScatChunks, sB);
                sB = ceil_div(numScatChunks, cpsB);
                const double cost = rounds((long long)(fullCT / kNumXcd) * numJGs * spEff) * (cps + 2.0) +
                                    rounds((long long)ceil_div(rem * sB, kNumXcd) * numJGs) * (cpsB + 2.0) + slabs + 3.0;   // + two more launches
                if (cost < bestCost) { bestCost = cost; p.scatSplit = spEff; p.scatChunksPerSplit = cps; p.scatRemCT = rem; p.scatRemSplit = sB; p.scatRemChunksPerSplit = cpsB; }
            }
        }
        p.scatDealPairs = numCT < kNumXcd || p.scatPerBlock;
    }
    p.NT = numScatChunks * kNC;
    const size_t npairs = (size_t)L * (L - 1) / 2;
    p.nFxPart = ceil_div(Lloc, 64) * ceil_div(p.numScanChunks, 4) * 4;
    p.nRegPart = (int)npairs + ceil_div(Lq, 256);
    p.grecvOff.assign(sWorld + 1, 0); p.xsendOff.assign(sWorld + 1, 0); p.xrecvOff.assign(sWorld + 1, 0);
    if (s.strips) {
        const size_t q2 = (size_t)q * q;
        size_t gtot = 0, stot = 0, rtot = 0;
        for (int r = 0; r < sWorld; ++r) {
            p.grecvOff[r] = gtot; p.xsendOff[r] = stot; p.xrecvOff[r] = rtot;
            if (r > sRank) { gtot += (size_t)LqLoc * plm_strip_cs(p.siteB, q, r); stot += (size_t)Lloc * (p.siteB[r + 1] - p.siteB[r]) * q2; }
            if (r < sRank) rtot += (size_t)(p.siteB[r + 1] - p.siteB[r]) * Lloc * q2;
        }
        p.grecvOff[sWorld] = gtot; p.xsendOff[sWorld] = stot; p.xrecvOff[sWorld] = rtot;
    }
    p.scatter = plm_scatter_stage(s, p, knobs);
    return p;
}

}  // namespace
