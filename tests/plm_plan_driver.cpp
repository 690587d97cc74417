// TEST INFRASTRUCTURE ONLY: the plmDCA engine's launch planner (pydca_amd/csrc/plm_plan.h, host code that PlmEngine::configure
// runs) behind a C call.  tests/test_plm_plan_host.py compiles it with the host compiler.  shape: the PlmShape fields in
// declaration order; knobs: the PlmKnobs fields in declaration order (-1 = unset); kernel_shapes: logits_seq_per_wg and
// logits_jt for q = 5, 21, 25.  out: the columns the test names, in its order; max_world bounds the per-rank columns.
#include "plm_plan.h"

extern "C" void plm_plan_driver(const int* shape, const int* knobs, const int* kernel_shapes, int max_world, long long* out)
{
    PlmShape s;
    s.N = shape[0]; s.L = shape[1]; s.q = shape[2]; s.elemBytes = shape[3]; s.halo = shape[4]; s.chunkArg = shape[5]; s.warmArg = shape[6];
    s.carryMode = shape[7]; s.stripWorld = shape[8]; s.stripRank = shape[9]; s.strips = shape[10] != 0;
    PlmKnobs k;
    k.scatterRem = knobs[0]; k.scatterSplit = knobs[1]; k.scatterCanon = knobs[2]; k.scatterWaves = knobs[3]; k.plmPairs = knobs[4];
    k.scatterMerge = knobs[5]; k.foldMerge = knobs[6]; k.fuseFx = knobs[7];
    const PlmKernelShapes ks{{kernel_shapes[0], kernel_shapes[1], kernel_shapes[2]}, {kernel_shapes[3], kernel_shapes[4], kernel_shapes[5]}};
    const PlmPlan p = plm_make_plan(s, k, ks);
    const int W = s.stripWorld;
    const long long v[] = {p.cS0, p.cS1, p.Lloc, (long long)p.oLo, (long long)p.oHi, p.pairBegin, p.pairEnd, p.chunk, p.warm, p.numScanChunks,
                           p.numScatChunks, (long long)p.P, p.Cs, p.pairs, p.gUnits, p.pairJT, p.Wrows, p.Grows, p.Npad, p.NT, p.scatJW, p.scatWaves,
                           p.scatSplit, p.scatChunksPerSplit, p.scatBlockChunks, p.scatPerBlock, p.scatRemCT, p.scatRemSplit, p.scatRemChunksPerSplit,
                           p.nFxPart, p.nRegPart, (long long)p.grecvOff[W], (long long)p.xsendOff[W], (long long)p.xrecvOff[W]};
    int n = 0;
    for (long long x : v) out[n++] = x;
    for (int r = 0; r <= max_world; ++r) out[n++] = r <= W ? p.siteB[r] : -1;
    for (const std::vector<size_t>* off : {&p.grecvOff, &p.xsendOff, &p.xrecvOff})
        for (int r = 0; r < max_world; ++r) out[n++] = r < W ? (long long)(*off)[r] : -1;
}
