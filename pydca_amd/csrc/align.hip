// Profile alignment of many sequences on the device (dca_profile_align, dca_sw_scores_device).
//
// One wave64 LANE aligns one query against the profile: the integer Gotoh recurrence
//     D[i][j] = max(D[i-1][j] + del_extend[i], H[i-1][j] + del_open[i])
//     I[i][j] = max(I[i][j-1] + ins_extend,    H[i][j-1] + ins_open)
//     H[i][j] = max(H[i-1][j-1] + match[i][s_j], D[i][j], I[i][j])        (local mode: also 0)
// runs in register strips of T profile columns: H and I of the previous residue j - 1 stay in VGPRs under a fully unrolled
// t loop, the vertical chain (H and D of column i - 1) runs through temporaries, a strip sweeps the whole query and only its
// right-edge column (H, D per residue) goes through device scratch, [j][lane].  The match table sits in LDS as [code][column],
// so a lane's T scores for its residue are contiguous 16-byte reads; del_open / del_extend of a strip are wave-uniform.
// With a traceback every cell leaves 4 pointer bits, packed over the strip into one 8- or 16-byte store per (strip, j, lane),
// and a second kernel, one lane per query, walks them back.  The host sorts the queries by length, cuts them into waves and
// passes (align_plan.h) and lays their codes out [j / 4][lane][4].
#include <algorithm>
#include <cstdlib>
#include <numeric>

#include "align_plan.h"
#include "dca_internal.h"

namespace {

struct AlignWave {
    int q0;                         // first query (position in the sorted order) of the wave
    int lanes;                      // queries of the wave: the lane stride of its three buffers
    int maxLen;                     // its longest query
    int pad;
    unsigned long long codeOff;     // dwords: codes[codeOff + (j / 4) * lanes + lane], byte j % 4
    unsigned long long edgeOff;     // int2:   edge[edgeOff + j * lanes + lane] = (H, D) of the last finished strip's right edge
    unsigned long long ptrOff;      // bytes:  ptr + ptrOff + ((strip * maxLen + j) * lanes + lane) * (T / 2)
};

struct AlignArgs {
    const int32_t* matchT;          // [A][LpPad]: the padded columns hold kAlignNeg (local) or 0 (glocal)
    const int32_t* delOpen;         // [LpPad], padded alike
    const int32_t* delExtend;
    const int32_t* h0;              // [LpPad + 1]: H[i][0] of the glocal boundary (unused in local mode)
    int insOpen, insExtend;
    int Lp, A, LpPad, strips, ldsStride, whole, nWaves;
    const AlignWave* waves;
    const int32_t* lens;            // sorted order
    const uint32_t* codes;
    int2* edge;
    uint8_t* ptr;
    int32_t* score;                 // sorted order
    int2* end;                      // (i, j) of the end cell, 1-based; sorted order
};

template <int T>
struct PtrWords;
template <>
struct PtrWords<16> { using type = uint2; };
template <>
struct PtrWords<32> { using type = uint4; };

// MODE: DCA_ALIGN_LOCAL / DCA_ALIGN_GLOCAL.  TRACE: pointer bits and the end cell are kept.
// Padded columns (i > Lp) only ever feed larger i, so the valid cells never see them: in local mode their tables hold kAlignNeg,
// which pins their H to 0 (they cannot raise the maximum); in glocal mode 0, which keeps them bounded, and they are not read.
template <int T, int MODE, bool TRACE>
__global__ __launch_bounds__(kAlignThreads)
void align_dp_kernel(AlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int32_t ldsMatch[];
    constexpr bool LOCAL = MODE == DCA_ALIGN_LOCAL;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * kAlignWaves + (threadIdx.x >> 6));
    AlignWave wv{};
    if (w < a.nWaves) wv = a.waves[w];              // a wave past the end keeps lanes = maxLen = 0 and only meets the barriers
    const int lanes = __builtin_amdgcn_readfirstlane(wv.lanes), maxLen = __builtin_amdgcn_readfirstlane(wv.maxLen);
    const bool mine = lane < lanes;
    const int len = mine ? a.lens[wv.q0 + lane] : 0;
    const uint32_t* codes = a.codes + wv.codeOff + lane;
    int2* edge = a.edge + wv.edgeOff + lane;
    const int stride = a.ldsStride, LpPad = a.LpPad;
    if (a.whole) {
        for (int k = threadIdx.x; k < a.A * LpPad; k += kAlignThreads) {
            const int c = k / LpPad, i = k - c * LpPad;
            ldsMatch[c * stride + i] = a.matchT[k];
        }
        __syncthreads();
    }
    const int insOpen = a.insOpen, insExtend = a.insExtend;
    int best = LOCAL ? 0 : a.h0[a.Lp], bi = LOCAL ? 0 : a.Lp, bj = 0;

    for (int s = 0; s < a.strips; ++s) {
        const int i0 = s * T;
        if (!a.whole) {
            __syncthreads();                        // every wave is done with the previous strip's slice
            for (int k = threadIdx.x; k < a.A * T; k += kAlignThreads) {
                const int c = k / T, t = k - c * T;
                ldsMatch[c * stride + t] = a.matchT[(size_t)c * LpPad + i0 + t];
            }
            __syncthreads();
        }
        const int32_t* table = a.whole ? ldsMatch + i0 : ldsMatch;
        const bool first = s == 0, last = s == a.strips - 1;
        const int tl = a.Lp - 1 - i0;               // the strip-local index of column Lp (last strip)
        int dO[T], dE[T], H[T], I[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            dO[t] = __builtin_amdgcn_readfirstlane(a.delOpen[i0 + t]);
            dE[t] = __builtin_amdgcn_readfirstlane(a.delExtend[i0 + t]);
            H[t] = LOCAL ? 0 : a.h0[i0 + t + 1];
            I[t] = kAlignNeg;
        }
        int diag = LOCAL ? 0 : a.h0[i0];            // H[i0][j - 1]
        uint32_t cw = 0, cwNext = (mine && maxLen > 0) ? codes[0] : 0u;
        int2 eNext = make_int2(0, kAlignNeg);       // row 0: H = 0, D = "minus infinity"
        if (!first && mine && maxLen > 0) eNext = edge[0];
        for (int j = 0; j < maxLen; ++j) {          // residue j + 1; the bound is wave-uniform
            if ((j & 3) == 0) {
                cw = cwNext;
                if (mine && j + 4 < maxLen) cwNext = codes[(size_t)((j >> 2) + 1) * lanes];
            }
            const int2 e = eNext;
            if (!first && mine && j + 1 < maxLen) eNext = edge[(size_t)(j + 1) * lanes];
            if (j < len) {
                const int code = (cw >> (8 * (j & 3))) & 0xff;
                const int4* mrow = reinterpret_cast<const int4*>(table + code * stride);
                int Hup = e.x, Dup = e.y, dg = diag, rowMax = 0;
                diag = e.x;
                uint32_t pw[T / 8];
#pragma unroll
                for (int k = 0; k < T / 8; ++k) pw[k] = 0;
#pragma unroll
                for (int t4 = 0; t4 < T / 4; ++t4) {
                    const int4 m4 = mrow[t4];
                    const int mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int t = t4 * 4 + u;
                        const int dOpenV = Hup + dO[t], iOpenV = H[t] + insOpen;
                        const int D = max(Dup + dE[t], dOpenV);
                        const int In = max(I[t] + insExtend, iOpenV);
                        const int hd = dg + mm[u];
                        int h = max(max(hd, D), In);
                        if (LOCAL) h = max(h, 0);
                        if (TRACE) {
                            uint32_t src = h == hd ? 1u : (h == D ? 2u : 3u);
                            if (LOCAL) src = h == 0 ? 0u : src;
                            const uint32_t nib = src | (D == dOpenV ? 4u : 0u) | (In == iOpenV ? 8u : 0u);
                            pw[t / 8] |= nib << (4 * (t % 8));
                        }
                        dg = H[t];
                        H[t] = h;
                        I[t] = In;
                        Hup = h;
                        Dup = D;
                        if (LOCAL) rowMax = max(rowMax, h);
                    }
                }
                if (!last) edge[(size_t)j * lanes] = make_int2(Hup, Dup);
                if (TRACE) {
                    using PW = typename PtrWords<T>::type;
                    PW* dst = reinterpret_cast<PW*>(a.ptr + wv.ptrOff) + ((size_t)s * maxLen + j) * lanes + lane;
                    PW v;
                    v.x = pw[0];
                    v.y = pw[1];
                    if constexpr (T == 32) { v.z = pw[2]; v.w = pw[3]; }
                    *dst = v;
                }
                if (LOCAL) {
                    if (!TRACE) best = max(best, rowMax);
                    else if (rowMax >= best) {
                        // the first maximum in row-major order (i outer): within the strip a later residue can reach it at a
                        // smaller column; earlier strips hold the smaller columns and are done
                        int tt = T - 1;
#pragma unroll
                        for (int t = T - 2; t >= 0; --t) tt = H[t] == rowMax ? t : tt;
                        const int i = i0 + tt + 1;
                        if (rowMax > best || i < bi) { best = rowMax; bi = i; bj = j + 1; }
                    }
                } else if (last) {
                    int hEnd = H[0];
#pragma unroll
                    for (int t = 1; t < T; ++t) hEnd = t == tl ? H[t] : hEnd;
                    if (hEnd > best) { best = hEnd; bj = j + 1; }     // the smallest j at the maximum
                }
            }
        }
    }
    if (mine) {
        a.score[wv.q0 + lane] = best;
        if (TRACE) a.end[wv.q0 + lane] = make_int2(bi, bj);
    }
}

// One lane per query walks its pointer bits from the end cell: in H the stored source (stop / diagonal / D / I), in D or I
// back to H when "open" was co-optimal.  residue_at (sorted order, prefilled with -1) gets the residue of every matched column.
template <int T, int MODE>
__global__ void align_trace_kernel(AlignArgs a, int nq, int32_t* __restrict__ residueAt)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nq) return;
    const AlignWave wv = a.waves[g >> 6];
    const int lane = g & 63;
    const uint8_t* ptr = a.ptr + wv.ptrOff;
    int32_t* out = residueAt + (size_t)g * a.Lp;
    const int2 e = a.end[wv.q0 + lane];
    int i = e.x, j = e.y, state = 0;
    while (i > 0 && j > 0) {
        const int c = i - 1, s = c / T, t = c - s * T;
        const size_t unit = ((size_t)s * wv.maxLen + (j - 1)) * wv.lanes + lane;
        const uint32_t nib = (ptr[unit * (T / 2) + (t >> 1)] >> (4 * (t & 1))) & 15u;
        if (state == 0) {
            const uint32_t src = nib & 3u;
            if (MODE == DCA_ALIGN_LOCAL && src == 0) break;
            if (src == 1) { out[c] = j - 1; --i; --j; }
            else state = src == 2 ? 1 : 2;
        } else if (state == 1) {
            if (nib & 4u) state = 0;
            --i;
        } else {
            if (nib & 8u) state = 0;
            --j;
        }
    }
}

template <int T, int MODE>
hipError_t launch_align(dca_ctx* ctx, const AlignArgs& a, size_t ldsBytes, bool trace)
{
    const dim3 grid((unsigned)ceil_div(a.nWaves, kAlignWaves));
    if (trace) hipLaunchKernelGGL((align_dp_kernel<T, MODE, true>), grid, dim3(kAlignThreads), ldsBytes, ctx->stream, a);
    else hipLaunchKernelGGL((align_dp_kernel<T, MODE, false>), grid, dim3(kAlignThreads), ldsBytes, ctx->stream, a);
    return hipGetLastError();
}

template <int T>
hipError_t launch_align_mode(dca_ctx* ctx, int mode, const AlignArgs& a, size_t ldsBytes, bool trace)
{
    return mode == DCA_ALIGN_LOCAL ? launch_align<T, DCA_ALIGN_LOCAL>(ctx, a, ldsBytes, trace)
                                   : launch_align<T, DCA_ALIGN_GLOCAL>(ctx, a, ldsBytes, trace);
}

template <int T>
hipError_t launch_trace(dca_ctx* ctx, int mode, const AlignArgs& a, int nq, int32_t* residueAt)
{
    const dim3 grid((unsigned)ceil_div(nq, 256));
    if (mode == DCA_ALIGN_LOCAL) hipLaunchKernelGGL((align_trace_kernel<T, DCA_ALIGN_LOCAL>), grid, dim3(256), 0, ctx->stream, a, nq, residueAt);
    else hipLaunchKernelGGL((align_trace_kernel<T, DCA_ALIGN_GLOCAL>), grid, dim3(256), 0, ctx->stream, a, nq, residueAt);
    return hipGetLastError();
}

}  // namespace

// The arguments are checked (capi.cpp: dca_profile_align).  scratch_bytes_out: the largest pass's edge columns + pointer bits.
int dca_profile_align_impl(dca_ctx* ctx, const int32_t* match, int Lp, int A, const int32_t* del_open, const int32_t* del_extend,
                           int ins_open, int ins_extend, int mode, const uint8_t* seqs, const int64_t* offsets, int n,
                           int32_t* score_out, int32_t* residue_at_out, unsigned long long* scratch_bytes_out)
{
    static const char* who = "dca_profile_align";
    const bool trace = residue_at_out != nullptr, local = mode == DCA_ALIGN_LOCAL;
    const AlignPlan plan = align_plan(Lp, A, trace);
    const int LpPad = plan.LpPad, padv = local ? kAlignNeg : 0;
    if (scratch_bytes_out) *scratch_bytes_out = 0;
    if (n == 0) return DCA_OK;

    // the tables as the kernel reads them: match transposed to [code][column], everything padded to whole strips
    std::vector<int32_t> tables((size_t)A * LpPad + 3 * (size_t)LpPad + 1, padv);
    int32_t* hMatchT = tables.data();
    int32_t* hOpen = hMatchT + (size_t)A * LpPad;
    int32_t* hExt = hOpen + LpPad;
    int32_t* hH0 = hExt + LpPad;
    for (int i = 0; i < Lp; ++i) {
        for (int c = 0; c < A; ++c) hMatchT[(size_t)c * LpPad + i] = match[(size_t)i * A + c];
        hOpen[i] = del_open[i];
        hExt[i] = del_extend[i];
    }
    hH0[0] = 0;
    for (int i = 1; i <= LpPad; ++i) hH0[i] = i > Lp ? 0 : (i == 1 ? del_open[0] : hH0[i - 1] + del_extend[i - 1]);

    std::vector<int32_t> lens((size_t)n), order((size_t)n);
    for (int k = 0; k < n; ++k) lens[k] = (int32_t)(offsets[k + 1] - offsets[k]);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lens[x] > lens[y]; });
    std::vector<int32_t> sortedLens((size_t)n);
    for (int k = 0; k < n; ++k) sortedLens[k] = lens[order[k]];

    const char* envPass = getenv("DCA_ALIGN_PASS");
    const long long passEnv = envPass ? atoll(envPass) : 0;

    DevBuf<int32_t> dTables, dLens, dScore, dResidue;
    DevBuf<AlignWave> dWaves;
    DevBuf<uint32_t> dCodes;
    DevBuf<int2> dEdge, dEnd;
    DevBuf<uint8_t> dPtr;
    HIP_TRY_AS_NOMEM(dTables.alloc(tables.size(), false), who);
    HIP_TRY_AS_NOMEM(dLens.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dScore.alloc((size_t)n, false), who);
    if (trace) HIP_TRY_AS_NOMEM(dEnd.alloc((size_t)n, false), who);
    HIP_TRY_AS(hipMemcpyAsync(dTables, tables.data(), tables.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS(hipMemcpyAsync(dLens, sortedLens.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), who);

    AlignArgs a{};
    a.matchT = dTables.get();
    a.delOpen = a.matchT + (size_t)A * LpPad;
    a.delExtend = a.delOpen + LpPad;
    a.h0 = a.delExtend + LpPad;
    a.insOpen = ins_open;
    a.insExtend = ins_extend;
    a.Lp = Lp;
    a.A = A;
    a.LpPad = LpPad;
    a.strips = plan.strips;
    a.ldsStride = plan.ldsStride;
    a.whole = plan.whole ? 1 : 0;
    a.lens = dLens.get();
    a.score = dScore.get();
    a.end = dEnd.get();

    std::vector<AlignWave> waves;
    std::vector<uint32_t> codes;
    std::vector<int32_t> residue;
    for (long long p0 = 0; p0 < n;) {
        const int nq = (int)std::min<long long>(n - p0, align_queries_per_pass(plan, sortedLens[p0], passEnv));
        waves.clear();
        unsigned long long codeDwords = 0, edgeUnits = 0, ptrBytes = 0;
        for (int k = 0; k < nq; k += 64) {
            AlignWave wv{};
            wv.q0 = (int)p0 + k;
            wv.lanes = std::min(64, nq - k);
            wv.maxLen = sortedLens[p0 + k];
            wv.codeOff = codeDwords;
            wv.edgeOff = edgeUnits;
            wv.ptrOff = ptrBytes;
            codeDwords += (unsigned long long)((wv.maxLen + 3) / 4) * wv.lanes;
            edgeUnits += (unsigned long long)wv.maxLen * wv.lanes;
            if (trace) ptrBytes += (unsigned long long)plan.strips * wv.maxLen * wv.lanes * (plan.T / 2);
            waves.push_back(wv);
        }
        codes.assign((size_t)std::max<unsigned long long>(codeDwords, 1), 0u);
        for (const AlignWave& wv : waves)
            for (int l = 0; l < wv.lanes; ++l) {
                const int src = order[wv.q0 + l];
                const uint8_t* r = seqs + offsets[src];
                uint8_t* dst = reinterpret_cast<uint8_t*>(codes.data() + wv.codeOff);
                for (int j = 0; j < lens[src]; ++j) dst[((size_t)(j >> 2) * wv.lanes + l) * 4 + (j & 3)] = r[j];
            }
        if (scratch_bytes_out) *scratch_bytes_out = std::max(*scratch_bytes_out, edgeUnits * sizeof(int2) + ptrBytes);
        HIP_TRY_AS_NOMEM(dWaves.alloc(waves.size(), false), who);
        HIP_TRY_AS_NOMEM(dCodes.alloc(codes.size(), false), who);
        HIP_TRY_AS_NOMEM(dEdge.alloc((size_t)std::max<unsigned long long>(edgeUnits, 1), false), who);
        if (trace) {
            HIP_TRY_AS_NOMEM(dPtr.alloc((size_t)std::max<unsigned long long>(ptrBytes, 16), false), who);
            HIP_TRY_AS_NOMEM(dResidue.alloc((size_t)nq * Lp, false), who);
            HIP_TRY_AS(hipMemsetAsync(dResidue, 0xff, (size_t)nq * Lp * sizeof(int32_t), ctx->stream), who);     // -1
        }
        HIP_TRY_AS(hipMemcpyAsync(dWaves, waves.data(), waves.size() * sizeof(AlignWave), hipMemcpyHostToDevice, ctx->stream), who);
        HIP_TRY_AS(hipMemcpyAsync(dCodes, codes.data(), codes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream), who);
        a.waves = dWaves.get();
        a.nWaves = (int)waves.size();
        a.codes = dCodes.get();
        a.edge = dEdge.get();
        a.ptr = dPtr.get();
        {
            ScopedKernelClock kc(ctx, "align_dp");
            HIP_TRY_AS(plan.T == 32 ? launch_align_mode<32>(ctx, mode, a, plan.ldsBytes, trace)
                                    : launch_align_mode<16>(ctx, mode, a, plan.ldsBytes, trace), who);
        }
        if (trace) {
            {
                ScopedKernelClock kc(ctx, "align_trace");
                HIP_TRY_AS(plan.T == 32 ? launch_trace<32>(ctx, mode, a, nq, dResidue.get()) : launch_trace<16>(ctx, mode, a, nq, dResidue.get()), who);
            }
            residue.resize((size_t)nq * Lp);
            HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
            HIP_TRY_AS(hipMemcpy(residue.data(), dResidue, residue.size() * sizeof(int32_t), hipMemcpyDeviceToHost), who);
            for (int k = 0; k < nq; ++k)
                memcpy(residue_at_out + (size_t)order[p0 + k] * Lp, residue.data() + (size_t)k * Lp, (size_t)Lp * sizeof(int32_t));
        } else {
            HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);      // the host vectors of this pass are reused by the next
        }
        p0 += nq;
    }
    std::vector<int32_t> sortedScore((size_t)n);
    HIP_TRY_AS(hipMemcpy(sortedScore.data(), dScore, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), who);
    for (int k = 0; k < n; ++k) score_out[order[k]] = sortedScore[k];
    return DCA_OK;
}
