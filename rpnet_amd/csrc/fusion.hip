// Label fusion of the masks R raters gave one volume (include/rpnet_fusion_abi.h): majority vote, weighted vote, binary STAPLE.
//
// A voxel enters every rule only through its decision pattern, the R-bit word of the raters that marked it.  So pass 1 writes the
// patterns and counts them (a 2^R-bin histogram), one block of 256 threads turns the histogram into a decision table label[p], w[p]
// (for STAPLE the whole EM runs there, on at most 4096 bins), and pass 2 maps patterns to the mask, the probability plane and the Dice
// counts.  Two passes over the volume whatever the iteration count.
//
// Bounds: every loop runs to a count fixed when it is entered (the trips of a block, the 16 voxels of a lane, the bins of a thread,
// max_iter).  Atomics are integer adds only (uint32 in LDS, 64-bit in memory), so their order does not reach the result.  No block
// waits for another; what a later launch reads, an earlier launch wrote.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "rpnet_fusion_abi.h"

namespace rpnet {
namespace {

typedef unsigned long long fus_u64;
constexpr int kFusLane = 16;                                    // voxels of a lane
constexpr int kFusBlocks = 1024;                                // most blocks of a pass; a block of 256 lanes owns 4096 voxels per trip
constexpr int kFusMaxBins = 1 << RPNET_FUSION_MAX_RATERS;       // 4096
constexpr int kFusBinsPerThread = kFusMaxBins / 256;            // 16
constexpr int kFusQ = RPNET_FUSION_MAX_RATERS;                  // row of Q_0 in the EM's sums: S1, S0, P_0.., then Q_0.. at 2 + kFusQ

struct FusRaters {
    const void* p[RPNET_FUSION_MAX_RATERS];
};
struct FusWeights {
    double w[RPNET_FUSION_MAX_RATERS];
};

static inline size_t fus_up16(size_t x) { return (x + 15) / 16 * 16; }
static inline bool fus_dims_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= RPNET_CC_MAX_DIM && H <= RPNET_CC_MAX_DIM && W <= RPNET_CC_MAX_DIM;
}
static inline size_t fus_need(int D, int H, int W, int R) {
    const size_t B = (size_t)1 << R, n = (size_t)D * H * W;
    return RPNET_FUSION_HEAD_BYTES + 16 * B + fus_up16(B) + fus_up16(2 * n);
}

// the voxels of a lane: 16-byte accesses where the lane is whole and its first address aligned; v[j] = 0 beyond cnt
template <class T>
__device__ __forceinline__ void fus_load16(const T* p, const size_t base, const int cnt, T (&v)[kFusLane]) {
    const T* q = p + base;
    if (cnt == kFusLane && ((uintptr_t)q & 15u) == 0) {
        uint4 w[sizeof(T)];                         // 16 elements are sizeof(T) words of 16 bytes
#pragma unroll
        for (int k = 0; k < (int)sizeof(T); ++k) w[k] = reinterpret_cast<const uint4*>(q)[k];
        __builtin_memcpy(v, w, sizeof(w));
    } else {
#pragma unroll
        for (int j = 0; j < kFusLane; ++j) v[j] = j < cnt ? q[j] : (T)0;
    }
}
template <class T>
__device__ __forceinline__ void fus_store16(T* p, const size_t base, const int cnt, const T (&v)[kFusLane]) {
    T* q = p + base;
    if (cnt == kFusLane && ((uintptr_t)q & 15u) == 0) {
        uint4 w[sizeof(T)];
        __builtin_memcpy(w, v, sizeof(w));
#pragma unroll
        for (int k = 0; k < (int)sizeof(T); ++k) reinterpret_cast<uint4*>(q)[k] = w[k];
    } else {
#pragma unroll
        for (int j = 0; j < kFusLane; ++j)
            if (j < cnt) q[j] = v[j];
    }
}

__device__ __forceinline__ unsigned fus_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ fus_u64 fus_wave_sum64(fus_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- pass 1
// grid `blocks` <= kFusBlocks; lane l of trip `it` owns the voxels [16 l, 16 l + 16), l = (it * blocks + block) * 256 + thread.
// Every lane of a wave runs every trip (cnt == 0 beyond the volume), so the ballots see whole waves.
template <class T>
__global__ __launch_bounds__(256) void fusion_pattern_kernel(const FusRaters ra, const int R, const T cls, uint16_t* __restrict__ patterns,
                                                             fus_u64* __restrict__ hist, const size_t n, const size_t n_lanes, const int iters) {
    __shared__ unsigned bins[kFusMaxBins];
    const int nb = 1 << R;
    const unsigned full = (unsigned)nb - 1u;
    for (int b = threadIdx.x; b < nb; b += 256) bins[b] = 0u;
    __syncthreads();
    unsigned c0 = 0u, c1 = 0u;          // the wave's voxels of pattern 0 and of pattern `full`: the same value in every lane
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)it * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
        const size_t base = lane * kFusLane;
        const int cnt = lane < n_lanes ? (int)min((size_t)kFusLane, n - base) : 0;
        uint16_t pat[kFusLane];
#pragma unroll
        for (int j = 0; j < kFusLane; ++j) pat[j] = 0;
#pragma unroll
        for (int r = 0; r < RPNET_FUSION_MAX_RATERS; ++r) {
            if (r < R) {
                T v[kFusLane];
                fus_load16(static_cast<const T*>(ra.p[r]), base, cnt, v);
#pragma unroll
                for (int j = 0; j < kFusLane; ++j) pat[j] |= (uint16_t)((v[j] == cls ? 1u : 0u) << r);
            }
        }
#pragma unroll
        for (int j = 0; j < kFusLane; ++j) {
            const bool valid = j < cnt;
            const bool zero = valid && pat[j] == 0, ones = valid && pat[j] == full;        // R >= 1: never both
            c0 += (unsigned)__popcll(__ballot(zero));
            c1 += (unsigned)__popcll(__ballot(ones));
            if (valid && !zero && !ones) atomicAdd(&bins[pat[j]], 1u);
        }
        fus_store16(patterns, base, cnt, pat);
    }
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(&bins[0], c0);
        if (c1) atomicAdd(&bins[full], c1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += 256) {
        const unsigned v = bins[b];
        if (v) atomicAdd(&hist[b], (fus_u64)v);
    }
}

// -------------------------------------------------------------------------------------------------------------- decision
// SUM of the header over `rows` rows of red at once: the thread's partials stand in red[row][t]; the result in red[row][0]
__device__ __forceinline__ void fus_tree(double (*red)[256], const int R, const int t) {
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] = __dadd_rn(red[0][t], red[0][t + s]);
            red[1][t] = __dadd_rn(red[1][t], red[1][t + s]);
            for (int r = 0; r < R; ++r) {
                red[2 + r][t] = __dadd_rn(red[2 + r][t], red[2 + r][t + s]);
                red[2 + kFusQ + r][t] = __dadd_rn(red[2 + kFusQ + r][t], red[2 + kFusQ + r][t + s]);
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ double fus_clamp(const double v) {
    const double lo = 0x1p-20, hi = 1.0 - 0x1p-20;
    return v < lo ? lo : (v > hi ? hi : v);
}

// one block of 256 threads; thread t owns the bins t + 256 k
__global__ __launch_bounds__(256) void fusion_decide_kernel(const long long* __restrict__ hist, const int R, const int method, const int min_votes,
                                                            const FusWeights wt, const int consensus, const int max_iter, const double tol,
                                                            uint8_t* __restrict__ label, double* __restrict__ wtab, long long* __restrict__ stats,
                                                            double* __restrict__ rater_f, long long* __restrict__ rater_i) {
    __shared__ double red[2 + 2 * kFusQ][256];
    __shared__ double sp[RPNET_FUSION_MAX_RATERS], sq[RPNET_FUSION_MAX_RATERS];
    __shared__ fus_u64 isum[4 + 2 * RPNET_FUSION_MAX_RATERS];       // n, num, voxels, n_fused, |rater_r and fused|.., |rater_r|..
    __shared__ int ctl[3];                                          // stop, iterations, converged
    const int t = threadIdx.x, nb = 1 << R, full = nb - 1;
    const bool staple = method == RPNET_FUSION_STAPLE;
    if (t < 4 + 2 * RPNET_FUSION_MAX_RATERS) isum[t] = 0ull;
    if (t < 3) ctl[t] = t == 2 ? 1 : 0;
    __syncthreads();

    long long h[kFusBinsPerThread];
    double w[kFusBinsPerThread];
    bool part[kFusBinsPerThread], lab[kFusBinsPerThread];
    fus_u64 l_n = 0, l_num = 0, l_vox = 0;
#pragma unroll
    for (int k = 0; k < kFusBinsPerThread; ++k) {
        const int p = t + 256 * k;
        const bool in = p < nb;
        h[k] = in ? hist[p] : 0ll;
        part[k] = in && !(staple && consensus && (p == 0 || p == full));
        w[k] = 0.0;
        lab[k] = false;
        l_vox += (fus_u64)h[k];
        if (part[k]) {
            l_n += (fus_u64)h[k];
            l_num += (fus_u64)h[k] * (fus_u64)__popc((unsigned)p);
        }
    }
    if (l_n) atomicAdd(&isum[0], l_n);
    if (l_num) atomicAdd(&isum[1], l_num);
    if (l_vox) atomicAdd(&isum[2], l_vox);
    __syncthreads();
    const long long n = (long long)isum[0], num = (long long)isum[1], voxels = (long long)isum[2];
    const bool em = staple && n > 0 && R > 1;

    if (!em) {
        const int mv = staple ? R : min_votes;
        double total = 0.0;
        for (int r = 0; r < R; ++r) total = __dadd_rn(total, wt.w[r]);
#pragma unroll
        for (int k = 0; k < kFusBinsPerThread; ++k) {
            const int p = t + 256 * k;
            if (p < nb) {
                if (method == RPNET_FUSION_WEIGHTED) {
                    double s = 0.0;
                    for (int r = 0; r < R; ++r)
                        if ((p >> r) & 1) s = __dadd_rn(s, wt.w[r]);
                    lab[k] = __dmul_rn(2.0, s) > total;
                    w[k] = __ddiv_rn(s, total);
                } else {
                    const int pc = __popc((unsigned)p);
                    lab[k] = pc >= mv;
                    w[k] = __ddiv_rn((double)pc, (double)R);
                }
            }
        }
    } else {
        const double g = __ddiv_rn((double)num, (double)((long long)R * n)), g1 = __dsub_rn(1.0, g);
        if (t < R) sp[t] = sq[t] = 0.99999;
        __syncthreads();
        for (int it = 0; it < max_iter; ++it) {
            red[0][t] = red[1][t] = 0.0;
            for (int r = 0; r < R; ++r) red[2 + r][t] = red[2 + kFusQ + r][t] = 0.0;
#pragma unroll
            for (int k = 0; k < kFusBinsPerThread; ++k) {
                if (part[k]) {
                    const int p = t + 256 * k;
                    double a = g, b = g1;
                    for (int r = 0; r < R; ++r) {
                        const bool d = (p >> r) & 1;
                        a = __dmul_rn(a, d ? sp[r] : __dsub_rn(1.0, sp[r]));
                        b = __dmul_rn(b, d ? __dsub_rn(1.0, sq[r]) : sq[r]);
                    }
                    w[k] = __ddiv_rn(a, __dadd_rn(a, b));
                    const double hd = (double)h[k];
                    const double hw = __dmul_rn(hd, w[k]), hv = __dmul_rn(hd, __dsub_rn(1.0, w[k]));
                    red[0][t] = __dadd_rn(red[0][t], hw);
                    red[1][t] = __dadd_rn(red[1][t], hv);
                    for (int r = 0; r < R; ++r) {
                        if ((p >> r) & 1)
                            red[2 + r][t] = __dadd_rn(red[2 + r][t], hw);
                        else
                            red[2 + kFusQ + r][t] = __dadd_rn(red[2 + kFusQ + r][t], hv);
                    }
                }
            }
            fus_tree(red, R, t);
            if (t == 0) {
                const double s1 = red[0][0], s0 = red[1][0];
                double delta = 0.0;
                for (int r = 0; r < R; ++r) {
                    const double po = sp[r], qo = sq[r];
                    const double pn = s1 != 0.0 ? fus_clamp(__ddiv_rn(red[2 + r][0], s1)) : po;
                    const double qn = s0 != 0.0 ? fus_clamp(__ddiv_rn(red[2 + kFusQ + r][0], s0)) : qo;
                    delta = fmax(delta, fmax(fabs(__dsub_rn(pn, po)), fabs(__dsub_rn(qn, qo))));
                    sp[r] = pn;
                    sq[r] = qn;
                }
                ctl[1] = it + 1;
                ctl[2] = delta < tol ? 1 : 0;
                ctl[0] = ctl[2];
            }
            __syncthreads();
            if (ctl[0]) break;          // the same word for every thread: the block leaves together
        }
#pragma unroll
        for (int k = 0; k < kFusBinsPerThread; ++k) {
            const int p = t + 256 * k;
            if (part[k])
                lab[k] = w[k] >= 0.5;
            else if (p < nb) {          // a consensus bin
                lab[k] = p == full;
                w[k] = p == full ? 1.0 : 0.0;
            }
        }
    }

    // the table, and the integer rows from hist and label: a thread's sums in registers, folded per wave, one LDS add per wave and row
    fus_u64 l_fused = 0, l_both[RPNET_FUSION_MAX_RATERS], l_mine[RPNET_FUSION_MAX_RATERS];
#pragma unroll
    for (int r = 0; r < RPNET_FUSION_MAX_RATERS; ++r) l_both[r] = l_mine[r] = 0ull;
#pragma unroll
    for (int k = 0; k < kFusBinsPerThread; ++k) {
        const int p = t + 256 * k;
        if (p < nb) {
            label[p] = lab[k] ? 1 : 0;
            wtab[p] = w[k];
            const fus_u64 hk = (fus_u64)h[k], hl = lab[k] ? hk : 0ull;
            l_fused += hl;
#pragma unroll
            for (int r = 0; r < RPNET_FUSION_MAX_RATERS; ++r) {
                if ((p >> r) & 1) {         // p < 2^R: no bit at or above R is set
                    l_both[r] += hl;
                    l_mine[r] += hk;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RPNET_FUSION_MAX_RATERS; ++r) {
        if (r < R) {                        // the same for every thread
            const fus_u64 both = fus_wave_sum64(l_both[r]), mine = fus_wave_sum64(l_mine[r]);
            if ((t & 63) == 0) {
                if (both) atomicAdd(&isum[4 + r], both);
                if (mine) atomicAdd(&isum[4 + RPNET_FUSION_MAX_RATERS + r], mine);
            }
        }
    }
    if (l_fused) atomicAdd(&isum[3], l_fused);
    __syncthreads();
    const long long n_fused = (long long)isum[3];
    if (t == 0) {
        stats[0] = n;
        stats[1] = n_fused;
        stats[2] = hist[full];
        stats[3] = voxels - hist[0] - hist[full];
        stats[4] = em ? ctl[1] : 0;
        stats[5] = em ? ctl[2] : 1;
    }
    if (t < R) {
        const long long both = (long long)isum[4 + t], mine = (long long)isum[4 + RPNET_FUSION_MAX_RATERS + t];
        rater_i[3 * t + 0] = both;
        rater_i[3 * t + 1] = mine;
        rater_i[3 * t + 2] = n_fused;
        if (em) {
            rater_f[2 * t + 0] = sp[t];
            rater_f[2 * t + 1] = sq[t];
        } else {
            const long long not_fused = voxels - n_fused, neither = voxels - mine - n_fused + both;
            rater_f[2 * t + 0] = n_fused ? __ddiv_rn((double)both, (double)n_fused) : 1.0;
            rater_f[2 * t + 1] = not_fused ? __ddiv_rn((double)neither, (double)not_fused) : 1.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- pass 2
// the lanes of pass 1.  truth may be null (then counts is); TT is the truth's element type
template <class TT>
__global__ __launch_bounds__(256) void fusion_apply_kernel(const uint16_t* __restrict__ patterns, const uint8_t* __restrict__ label,
                                                           const double* __restrict__ wtab, const int nb, uint8_t* out, const uint8_t cls,
                                                           const int merge, float* __restrict__ prob, const TT* __restrict__ truth, const TT tcls,
                                                           fus_u64* __restrict__ counts, const size_t n, const size_t n_lanes, const int iters) {
    __shared__ uint8_t slab[kFusMaxBins];
    __shared__ float sw[kFusMaxBins];
    __shared__ unsigned cnt3[3];
    for (int b = threadIdx.x; b < nb; b += 256) {
        slab[b] = label[b];
        if (prob) sw[b] = (float)wtab[b];
    }
    if (threadIdx.x < 3) cnt3[threadIdx.x] = 0u;
    __syncthreads();
    unsigned c_pt = 0u, c_p = 0u, c_t = 0u;
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)it * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
        const size_t base = lane * kFusLane;
        const int cnt = lane < n_lanes ? (int)min((size_t)kFusLane, n - base) : 0;
        if (cnt == 0) continue;
        uint16_t pat[kFusLane];
        fus_load16(patterns, base, cnt, pat);
        uint8_t o[kFusLane];
        if (merge) {
            fus_load16(out, base, cnt, o);
#pragma unroll
            for (int j = 0; j < kFusLane; ++j)
                if (o[j] == 0 && slab[pat[j]]) o[j] = cls;
        } else {
#pragma unroll
            for (int j = 0; j < kFusLane; ++j) o[j] = slab[pat[j]] ? cls : (uint8_t)0;
        }
        fus_store16(out, base, cnt, o);
        if (prob) {
            float pr[kFusLane];
#pragma unroll
            for (int j = 0; j < kFusLane; ++j) pr[j] = sw[pat[j]];
            fus_store16(prob, base, cnt, pr);
        }
        if (truth) {
            TT tv[kFusLane];
            fus_load16(truth, base, cnt, tv);
#pragma unroll
            for (int j = 0; j < kFusLane; ++j) {
                if (j < cnt) {
                    const bool P = o[j] == cls, T = tv[j] == tcls;
                    c_pt += (P && T) ? 1u : 0u;
                    c_p += P ? 1u : 0u;
                    c_t += T ? 1u : 0u;
                }
            }
        }
    }
    if (counts) {           // the same for every thread
        c_pt = fus_wave_sum(c_pt);
        c_p = fus_wave_sum(c_p);
        c_t = fus_wave_sum(c_t);
        if ((threadIdx.x & 63) == 0) {
            if (c_pt) atomicAdd(&cnt3[0], c_pt);
            if (c_p) atomicAdd(&cnt3[1], c_p);
            if (c_t) atomicAdd(&cnt3[2], c_t);
        }
        __syncthreads();
        if (threadIdx.x < 3 && cnt3[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (fus_u64)cnt3[threadIdx.x]);
    }
}

struct FusGrid {
    size_t n, n_lanes;
    int blocks, iters;
};
static inline FusGrid fus_grid(int D, int H, int W) {
    FusGrid g;
    g.n = (size_t)D * H * W;
    g.n_lanes = (g.n + kFusLane - 1) / kFusLane;
    g.blocks = (int)std::min<size_t>((g.n_lanes + 255) / 256, (size_t)kFusBlocks);
    g.iters = (int)((g.n_lanes + (size_t)g.blocks * 256 - 1) / ((size_t)g.blocks * 256));
    return g;
}

const size_t kFusElem[4] = {1, 4, 8, 4};

// the refusals pass 1 needs, shared by the two entry points
static int fus_check_raters(const char* fn, const void* const* raters, int R, int kind, int cls, int D, int H, int W) {
    RPNET_REQUIRE(R >= 1 && R <= RPNET_FUSION_MAX_RATERS, RPNET_ERR_ARG, "%s: R=%d (1..%d raters)", fn, R, RPNET_FUSION_MAX_RATERS);
    RPNET_REQUIRE(raters, RPNET_ERR_ARG, "%s: null pointer", fn);
    for (int r = 0; r < R; ++r) RPNET_REQUIRE(raters[r], RPNET_ERR_ARG, "%s: null pointer (rater %d)", fn, r);
    RPNET_REQUIRE(kind >= RPNET_CC_U8 && kind <= RPNET_CC_F32, RPNET_ERR_ARG, "%s: element kind %d (0 uint8, 1 int32, 2 int64, 3 float32)", fn, kind);
    RPNET_REQUIRE(cls >= 1 && cls <= 255, RPNET_ERR_ARG, "%s: class %d (1..255)", fn, cls);
    RPNET_REQUIRE(fus_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    for (int r = 0; r < R; ++r)
        RPNET_REQUIRE(((uintptr_t)raters[r] % kFusElem[kind]) == 0, RPNET_ERR_ARG, "%s: rater %d is not aligned to its element", fn, r);
    return 0;
}

// every argument has been checked; hist has been cleared on `st`
static void fus_launch_patterns(const void* const* raters, int R, int kind, int cls, int D, int H, int W, uint16_t* patterns, fus_u64* hist,
                                hipStream_t st) {
    FusRaters ra;
    for (int r = 0; r < RPNET_FUSION_MAX_RATERS; ++r) ra.p[r] = r < R ? raters[r] : nullptr;
    const FusGrid g = fus_grid(D, H, W);
    const dim3 grid(g.blocks), block(256);
    switch (kind) {
        case RPNET_CC_U8:
            hipLaunchKernelGGL(fusion_pattern_kernel<uint8_t>, grid, block, 0, st, ra, R, (uint8_t)cls, patterns, hist, g.n, g.n_lanes, g.iters);
            break;
        case RPNET_CC_I32:
            hipLaunchKernelGGL(fusion_pattern_kernel<int32_t>, grid, block, 0, st, ra, R, (int32_t)cls, patterns, hist, g.n, g.n_lanes, g.iters);
            break;
        case RPNET_CC_I64:
            hipLaunchKernelGGL(fusion_pattern_kernel<int64_t>, grid, block, 0, st, ra, R, (int64_t)cls, patterns, hist, g.n, g.n_lanes, g.iters);
            break;
        default:
            hipLaunchKernelGGL(fusion_pattern_kernel<float>, grid, block, 0, st, ra, R, (float)cls, patterns, hist, g.n, g.n_lanes, g.iters);
    }
}

template <class TT>
static void fus_launch_apply(const FusGrid& g, const uint16_t* patterns, const uint8_t* label, const double* wtab, int nb, uint8_t* out, int cls,
                             int merge, float* prob, const void* truth, fus_u64* counts, hipStream_t st) {
    hipLaunchKernelGGL(fusion_apply_kernel<TT>, dim3(g.blocks), dim3(256), 0, st, patterns, label, wtab, nb, out, (uint8_t)cls, merge, prob,
                       static_cast<const TT*>(truth), (TT)cls, counts, g.n, g.n_lanes, g.iters);
}

}  // namespace
}  // namespace rpnet

extern "C" int rpnet_fusion_abi_version(void) { return RPNET_FUSION_ABI_VERSION; }

extern "C" size_t rpnet_fusion_workspace_bytes(int D, int H, int W, int R) {
    using namespace rpnet;
    if (!fus_dims_ok(D, H, W) || R < 1 || R > RPNET_FUSION_MAX_RATERS) {
        set_error("fusion_workspace_bytes: D=%d H=%d W=%d R=%d (every extent 1..%d, R 1..%d)", D, H, W, R, RPNET_CC_MAX_DIM, RPNET_FUSION_MAX_RATERS);
        return 0;
    }
    return fus_need(D, H, W, R);
}

extern "C" int rpnet_fusion_patterns(const void* const* raters, int R, int kind, int cls, int D, int H, int W, uint16_t* patterns, int64_t* hist,
                                     rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "fusion_patterns";
    if (const int rc = fus_check_raters(fn, raters, R, kind, cls, D, H, W)) return rc;
    RPNET_REQUIRE(patterns && hist, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(((uintptr_t)patterns % 2) == 0 && ((uintptr_t)hist % 8) == 0, RPNET_ERR_ARG,
                  "%s: patterns must be aligned to 2 and hist to 8 bytes", fn);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, sizeof(int64_t) << R, st) != hipSuccess) return check_launch(fn);
    fus_launch_patterns(raters, R, kind, cls, D, H, W, patterns, reinterpret_cast<fus_u64*>(hist), st);
    return check_launch(fn);
}

extern "C" int rpnet_fusion_fuse(const void* const* raters, int R, int kind, int cls, int D, int H, int W, int method, int min_votes,
                                 const double* weights, int consensus, int max_iter, double tol, uint8_t* out, int merge, float* prob,
                                 const void* truth, int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats, double* rater_f,
                                 int64_t* rater_i, int64_t row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "fusion_fuse";
    if (const int rc = fus_check_raters(fn, raters, R, kind, cls, D, H, W)) return rc;
    RPNET_REQUIRE(out && stats && rater_f && rater_i && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE((truth == nullptr) == (counts == nullptr), RPNET_ERR_ARG, "%s: truth and counts come together (both or neither)", fn);
    RPNET_REQUIRE(!truth || (truth_kind >= RPNET_CC_U8 && truth_kind <= RPNET_CC_F32), RPNET_ERR_ARG,
                  "%s: element kind %d of truth (0 uint8, 1 int32, 2 int64, 3 float32)", fn, truth_kind);
    RPNET_REQUIRE(method >= RPNET_FUSION_VOTE && method <= RPNET_FUSION_STAPLE, RPNET_ERR_ARG, "%s: method %d (0 vote, 1 weighted, 2 staple)", fn,
                  method);
    RPNET_REQUIRE(min_votes >= 1 && min_votes <= R, RPNET_ERR_ARG, "%s: min_votes %d (1..R = %d)", fn, min_votes, R);
    FusWeights wt;
    for (int r = 0; r < RPNET_FUSION_MAX_RATERS; ++r) wt.w[r] = 0.0;
    if (method == RPNET_FUSION_WEIGHTED) {
        RPNET_REQUIRE(weights, RPNET_ERR_ARG, "%s: the weighted vote needs weights", fn);
        double total = 0.0;
        for (int r = 0; r < R; ++r) {
            RPNET_REQUIRE(std::isfinite(weights[r]) && weights[r] >= 0.0, RPNET_ERR_ARG, "%s: weight %d is %g (every weight finite and >= 0)", fn, r,
                          weights[r]);
            wt.w[r] = weights[r];
            total += weights[r];
        }
        RPNET_REQUIRE(std::isfinite(total) && total > 0.0, RPNET_ERR_ARG, "%s: the weights add up to %g (a finite total > 0)", fn, total);
    }
    RPNET_REQUIRE(max_iter >= 1 && max_iter <= RPNET_FUSION_MAX_ITER, RPNET_ERR_ARG, "%s: max_iter %d (1..%d)", fn, max_iter, RPNET_FUSION_MAX_ITER);
    RPNET_REQUIRE(tol >= 0.0, RPNET_ERR_ARG, "%s: tol is %g (>= 0)", fn, tol);         // a NaN fails the comparison
    RPNET_REQUIRE(n_rows >= 1 && row >= 0 && row < n_rows && (!counts || (counts_row >= 0 && counts_row < n_rows)), RPNET_ERR_ARG,
                  "%s: rows %lld and %lld of tables of %lld rows", fn, (long long)counts_row, (long long)row, (long long)n_rows);
    const size_t need = fus_need(D, H, W, R);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    RPNET_REQUIRE((!truth || ((uintptr_t)truth % kFusElem[truth_kind]) == 0) && ((uintptr_t)prob % 4) == 0 && ((uintptr_t)stats % 8) == 0 &&
                      ((uintptr_t)rater_f % 8) == 0 && ((uintptr_t)rater_i % 8) == 0 && ((uintptr_t)counts % 8) == 0 &&
                      ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: volumes must be aligned to their element, the tables to 8 and the workspace to 16 bytes", fn);
    const FusGrid g = fus_grid(D, H, W);
    for (int r = 0; r < R; ++r) {
        const uintptr_t a0 = (uintptr_t)raters[r], a1 = a0 + g.n * kFusElem[kind], b0 = (uintptr_t)out, b1 = b0 + g.n;
        RPNET_REQUIRE(a1 <= b0 || b1 <= a0, RPNET_ERR_ARG, "%s: out overlaps rater %d", fn, r);
    }

    const size_t B = (size_t)1 << R;
    char* ws = static_cast<char*>(workspace);
    fus_u64* hist = reinterpret_cast<fus_u64*>(ws + RPNET_FUSION_HEAD_BYTES);
    double* wtab = reinterpret_cast<double*>(ws + RPNET_FUSION_HEAD_BYTES + 8 * B);
    uint8_t* label = reinterpret_cast<uint8_t*>(ws + RPNET_FUSION_HEAD_BYTES + 16 * B);
    uint16_t* patterns = reinterpret_cast<uint16_t*>(ws + RPNET_FUSION_HEAD_BYTES + 16 * B + fus_up16(B));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, RPNET_FUSION_HEAD_BYTES + 8 * B, st) != hipSuccess) return check_launch(fn);
    fus_launch_patterns(raters, R, kind, cls, D, H, W, patterns, hist, st);
    hipLaunchKernelGGL(fusion_decide_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const long long*>(hist), R, method, min_votes, wt,
                       consensus != 0 ? 1 : 0, max_iter, tol, label, wtab, reinterpret_cast<long long*>(stats) + row * RPNET_FUSION_STATS_ROW,
                       rater_f + row * R * 2, reinterpret_cast<long long*>(rater_i) + row * R * 3);
    fus_u64* crow = counts ? reinterpret_cast<fus_u64*>(counts) + counts_row * RPNET_FUSION_COUNTS_ROW : nullptr;
    const int nb = (int)B, mg = merge != 0 ? 1 : 0;
    switch (truth ? truth_kind : RPNET_CC_U8) {
        case RPNET_CC_U8: fus_launch_apply<uint8_t>(g, patterns, label, wtab, nb, out, cls, mg, prob, truth, crow, st); break;
        case RPNET_CC_I32: fus_launch_apply<int32_t>(g, patterns, label, wtab, nb, out, cls, mg, prob, truth, crow, st); break;
        case RPNET_CC_I64: fus_launch_apply<int64_t>(g, patterns, label, wtab, nb, out, cls, mg, prob, truth, crow, st); break;
        default: fus_launch_apply<float>(g, patterns, label, wtab, nb, out, cls, mg, prob, truth, crow, st);
    }
    return check_launch(fn);
}
