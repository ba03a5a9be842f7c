// Surface distances of an evaluated volume on a grid with a per-axis voxel spacing (include/rpnet_surface_spacing_abi.h;
// rpnet_amd/surface_spacing.py): the tallies behind HD95, HD, ASSD and NSD in millimetres.  The transform is that of surface.hip
// (surface_edt.h) under another metric: the squared distance of a voxel is ((wx*dx^2 + wy*dy^2) + wz*dz^2) in fp64.  Every product and every sum is one rounding (__dmul_rn / __dadd_rn, and the file is built with
// -ffp-contract=off), every squared offset an exact integer, and a minimum does not depend on the order of its candidates: a numpy
// restatement of the same operations gets the same bits.
//
// Launches of a tally: clear (head), x pass, y pass, z pass, statistics, eight radix passes, finalize; their number and shape depend on
// (D, H, W) alone.  The values are no longer small integers, so the order statistics come from a most-significant-digit radix selection
// over the bit patterns (non-negative doubles order like their bits read as uint64) instead of a histogram over d^2.  Bounds: every loop
// runs to a count fixed when it is entered; no thread waits on another block; blocks share nothing but integer atomics; the sums of
// square roots are per-block partial sums written by block index and combined in index order by one block.  The head is cleared by a
// launch of its own, not by hipMemsetAsync: captured in a graph, the memset node of this head filled it with stale bytes from the second
// replay on (the words no kernel writes came back non-zero), while a kernel's arguments are part of its node.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "rpnet_surface_spacing_abi.h"
#include "surface_edt.h"

namespace rpnet {

typedef unsigned long long sps_u64;

constexpr int kSpsBlocks = 2048;                                // blocks of the statistics and radix launches at most
constexpr int kSpsPasses = 8, kSpsDigit = 256;                  // 8 passes of 8 bits
// head of the workspace, in 8-byte words
constexpr int kSpsCnt = 0;                                      // n_A, n_B, within_A, within_B, bits of the largest d2
constexpr int kSpsState = 8;                                    // [pass][prefix of rank k, of rank k1, remaining rank k, k1]
constexpr int kSpsHist = kSpsState + 4 * kSpsPasses + 24;       // = 64: [pass][rank][digit]
constexpr int kSpsHeadWords = kSpsHist + kSpsPasses * 2 * kSpsDigit;
constexpr size_t kSpsHeadBytes = (size_t)kSpsHeadWords * 8;     // cleared by the first launch
constexpr size_t kSpsPartBytes = (size_t)2 * kSpsBlocks * 8;    // partial sums [A, B][block]: every used entry is written before it is read
static_assert(kSpsHist == 64 && kSpsHeadBytes % 16 == 0 && kSpsPartBytes % 16 == 0, "the volumes behind the head stay 16-byte aligned");
static_assert(RPNET_SURFACE_SPACING_MAX_DIM == RPNET_SURFACE_MAX_DIM, "the extent limit of the integer path");

struct SpsMetric {                                              // w * o^2 along one axis: one rounding per product and per sum
    typedef double T;
    double w;                                                   // the weight of the axis of the pass
    static constexpr T kNoSeed = DBL_MAX;                       // finite, above every reachable distance; DBL_MAX + w*o^2 never goes below it
    static constexpr int kTileBytes = 32 * 1024;                // LDS of a y / z tile while its rows stay at least kMinTile columns wide
    static constexpr int kMaxTile = 32, kMinTile = 8;           // 256-byte rows at most, 64-byte rows at least: 64 KiB of LDS for lines above 512
    __device__ __forceinline__ T cost(const int o) const { return __dmul_rn(w, (double)(o * o)); }
    static __device__ __forceinline__ T add(const T a, const T b) { return __dadd_rn(a, b); }
    static __device__ __forceinline__ T lower(const T a, const T b) { return fmin(a, b); }
};
static_assert((size_t)RPNET_SURFACE_SPACING_MAX_DIM * SpsMetric::kMinTile * sizeof(double) <= 64 * 1024, "the longest line, narrowest tile: 64 KiB");

// the memset of the head: counters, selection states and radix histograms to 0; grid ceil(kSpsHeadWords / 256)
__global__ __launch_bounds__(256) void surface_spacing_clear_kernel(sps_u64* __restrict__ head) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < kSpsHeadWords) head[i] = 0ull;
}

// n_A, n_B, the NSD counts, the largest squared distance and the partial sums of square roots.  A voxel is on a border exactly where
// that volume's transform is 0 (the weights are > 0).  `iters` grid-sized sweeps cover the n voxels.  part[blockIdx.x] and
// part[kSpsBlocks + blockIdx.x]: the block's sums over border(A) and border(B), each thread in sweep order, then a fixed tree.
__global__ __launch_bounds__(256) void surface_spacing_stats_kernel(const double* __restrict__ gA, const double* __restrict__ gB, const size_t n,
                                                                    const int iters, const double tau2, sps_u64* __restrict__ head,
                                                                    double* __restrict__ part) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned lc[4];
    __shared__ sps_u64 lmax;
    __shared__ double pa[256], pb[256];
    const int t = threadIdx.x;
    if (t < 4) lc[t] = 0u;
    if (t == 0) lmax = 0ull;
    __syncthreads();
    double fa = 0.0, fb = 0.0;
    sps_u64 mx = 0ull;
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)it * gridDim.x + blockIdx.x) * 256u + t;
        double a = 1.0, b = 1.0;
        if (i < n) {
            a = gA[i];
            b = gB[i];
        }
        if (a == 0.0) {
            atomicAdd(&lc[0], 1u);
            if (b <= tau2) atomicAdd(&lc[2], 1u);
            fa = __dadd_rn(fa, sqrt(b));
            mx = max(mx, (sps_u64)__double_as_longlong(b));
        }
        if (b == 0.0) {
            atomicAdd(&lc[1], 1u);
            if (a <= tau2) atomicAdd(&lc[3], 1u);
            fb = __dadd_rn(fb, sqrt(a));
            mx = max(mx, (sps_u64)__double_as_longlong(a));
        }
    }
    pa[t] = fa;
    pb[t] = fb;
    if (mx) atomicMax(&lmax, mx);
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            pa[t] = __dadd_rn(pa[t], pa[t + d]);
            pb[t] = __dadd_rn(pb[t], pb[t + d]);
        }
        __syncthreads();
    }
    if (t < 4 && lc[t]) atomicAdd(head + kSpsCnt + t, (sps_u64)lc[t]);
    if (t == 0) {
        if (lmax) atomicMax(head + kSpsCnt + 4, lmax);
        part[blockIdx.x] = pa[0];
        part[kSpsBlocks + blockIdx.x] = pb[0];
    }
}

// numpy's percentile: virtual index (n - 1) * (95 / 100), then floor
__device__ __forceinline__ long long sps_rank(const sps_u64 n) { return (long long)floor(0.95 * (double)(n - 1)); }

// One step of the selection, by a whole block of 256 threads: from the state at the entry of pass `p` (prefix and remaining rank of
// either rank q) and the histogram that pass counted, the state at its exit into sp[q], sr[q].  The remaining rank is below the count
// of the values under the prefix, so exactly one digit owns it.  scan: [2][256] of LDS.
__device__ __forceinline__ void sps_pick(const sps_u64* __restrict__ head, const int p, sps_u64* sp, sps_u64* sr, sps_u64 (*scan)[kSpsDigit]) {
    const int t = threadIdx.x, shift = 56 - 8 * p;
    const sps_u64* __restrict__ st = head + kSpsState + 4 * p;
    const sps_u64* __restrict__ hist = head + kSpsHist + (size_t)p * 2 * kSpsDigit;
    const sps_u64 own[2] = {hist[t], hist[kSpsDigit + t]};
    scan[0][t] = own[0];
    scan[1][t] = own[1];
    if (t < 2) {
        sp[t] = st[t];
        sr[t] = 0ull;
    }
    __syncthreads();
    for (int d = 1; d < kSpsDigit; d <<= 1) {       // inclusive prefix sums over the digits
        const sps_u64 v0 = t >= d ? scan[0][t - d] : 0ull, v1 = t >= d ? scan[1][t - d] : 0ull;
        __syncthreads();
        scan[0][t] += v0;
        scan[1][t] += v1;
        __syncthreads();
    }
    for (int q = 0; q < 2; ++q) {
        const sps_u64 incl = scan[q][t], excl = incl - own[q], r = st[2 + q];
        if (excl <= r && r < incl) {
            sp[q] = st[q] | ((sps_u64)t << shift);
            sr[q] = r - excl;
        }
    }
    __syncthreads();
}

// Radix pass p (digit = bits [56 - 8p, 64 - 8p) of the key): the state at its entry is formed from pass p - 1 (block 0 stores it for
// the pass after), then hist[p][q][digit] += 1 for every pooled value whose bits above the digit equal the prefix of rank q.
__global__ __launch_bounds__(256) void surface_spacing_radix_kernel(const double* __restrict__ gA, const double* __restrict__ gB, const size_t n,
                                                                    const int iters, const int p, sps_u64* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned lh[2][kSpsDigit];
    __shared__ sps_u64 scan[2][kSpsDigit];
    __shared__ sps_u64 sp[2], sr[2];
    const int t = threadIdx.x;
    const sps_u64 nA = head[kSpsCnt], nB = head[kSpsCnt + 1];
    if (nA == 0 || nB == 0) return;                                 // block-uniform
    lh[0][t] = 0u;
    lh[1][t] = 0u;
    if (p == 0) {
        if (t == 0) {
            const sps_u64 cnt = nA + nB;
            const long long k = sps_rank(cnt);
            sp[0] = sp[1] = 0ull;
            sr[0] = (sps_u64)k;
            sr[1] = (sps_u64)min(k + 1, (long long)cnt - 1);
        }
        __syncthreads();
    } else {
        sps_pick(head, p - 1, sp, sr, scan);
    }
    if (blockIdx.x == 0 && t < 2) {
        head[kSpsState + 4 * p + t] = sp[t];
        head[kSpsState + 4 * p + 2 + t] = sr[t];
    }
    const int shift = 56 - 8 * p;
    const sps_u64 pre0 = sp[0], pre1 = sp[1];
    const sps_u64 above = p == 0 ? 0ull : ~0ull << (shift + 8);     // the bits a prefix fixes
    const bool same = pre0 == pre1;
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)it * gridDim.x + blockIdx.x) * 256u + t;
        double a = 1.0, b = 1.0;
        if (i < n) {
            a = gA[i];
            b = gB[i];
        }
        for (int side = 0; side < 2; ++side) {
            if ((side ? b : a) != 0.0) continue;
            const sps_u64 key = (sps_u64)__double_as_longlong(side ? a : b);
            const unsigned digit = (unsigned)(key >> shift) & (kSpsDigit - 1);
            if ((key & above) == pre0) atomicAdd(&lh[0][digit], 1u);
            if (!same && (key & above) == pre1) atomicAdd(&lh[1][digit], 1u);
        }
    }
    __syncthreads();
    sps_u64* __restrict__ hist = head + kSpsHist + (size_t)p * 2 * kSpsDigit;
    const unsigned c0 = lh[0][t], c1 = same ? c0 : lh[1][t];
    if (c0) atomicAdd(hist + t, (sps_u64)c0);
    if (c1) atomicAdd(hist + kSpsDigit + t, (sps_u64)c1);
}

// One block: the last digit of either rank, the partial sums combined in index order (thread t owns `per` consecutive blocks, thread 0
// combines the 256 results in thread order), and the two rows.
__global__ __launch_bounds__(256) void surface_spacing_finalize_kernel(const sps_u64* __restrict__ head, const double* __restrict__ part,
                                                                       const int nblocks, const int per, long long* __restrict__ irow,
                                                                       double* __restrict__ frow) {
    RPNET_PASS_PRIORITY();
    __shared__ sps_u64 scan[2][kSpsDigit];
    __shared__ sps_u64 sp[2], sr[2];
    __shared__ double pf[2][256];
    const int t = threadIdx.x;
    const sps_u64 nA = head[kSpsCnt], nB = head[kSpsCnt + 1];
    if (nA == 0 || nB == 0) {                                       // block-uniform
        if (t < RPNET_SURFACE_SPACING_IROW) irow[t] = t == 2 ? -1 : 0;
        if (t < RPNET_SURFACE_SPACING_FROW) frow[t] = 0.0;
        return;
    }
    sps_pick(head, kSpsPasses - 1, sp, sr, scan);
    const int lo = min(t * per, nblocks), hi = min(lo + per, nblocks);
    double fa = 0.0, fb = 0.0;
    for (int b = lo; b < hi; ++b) {
        fa = __dadd_rn(fa, part[b]);
        fb = __dadd_rn(fb, part[kSpsBlocks + b]);
    }
    pf[0][t] = fa;
    pf[1][t] = fb;
    __syncthreads();
    if (t == 0) {
        double sa = 0.0, sb = 0.0;
        for (int j = 0; j < 256; ++j) {
            sa = __dadd_rn(sa, pf[0][j]);
            sb = __dadd_rn(sb, pf[1][j]);
        }
        irow[0] = (long long)nA;
        irow[1] = (long long)nB;
        irow[2] = sps_rank(nA + nB);
        irow[3] = (long long)head[kSpsCnt + 2];
        irow[4] = (long long)head[kSpsCnt + 3];
        frow[0] = __longlong_as_double((long long)sp[0]);
        frow[1] = __longlong_as_double((long long)sp[1]);
        frow[2] = __longlong_as_double((long long)head[kSpsCnt + 4]);
        frow[3] = sa;
        frow[4] = sb;
    }
}

}  // namespace rpnet

extern "C" int rpnet_surface_spacing_abi_version(void) { return RPNET_SURFACE_SPACING_ABI_VERSION; }

extern "C" size_t rpnet_surface_spacing_workspace_bytes(int D, int H, int W) {
    using namespace rpnet;
    if (D < 1 || H < 1 || W < 1 || D > RPNET_SURFACE_SPACING_MAX_DIM || H > RPNET_SURFACE_SPACING_MAX_DIM || W > RPNET_SURFACE_SPACING_MAX_DIM) {
        set_error("surface_spacing: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_SURFACE_SPACING_MAX_DIM);
        return 0;
    }
    return kSpsHeadBytes + kSpsPartBytes + 2 * (size_t)D * H * W * sizeof(double);
}

extern "C" int rpnet_surface_spacing_tally(const void* pred, int pred_kind, const void* truth, int truth_kind, int cls, int D, int H, int W,
                                           const double* w, double tau2, int64_t* itable, int64_t irow, double* ftable, int64_t frow,
                                           int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(w, RPNET_ERR_ARG, "surface_spacing_tally: null pointer");
    if (const int rc = surface_check_tally("surface_spacing_tally", pred, pred_kind, truth, truth_kind, D, H, W, itable, irow, ftable, frow,
                                           n_rows, workspace, workspace_bytes, rpnet_surface_spacing_workspace_bytes))
        return rc;
    for (int a = 0; a < 3; ++a)
        RPNET_REQUIRE(std::isfinite(w[a]) && w[a] > 0.0, RPNET_ERR_ARG, "surface_spacing_tally: weight %d is %g (every weight finite and > 0)", a,
                      w[a]);
    RPNET_REQUIRE(!std::isnan(tau2), RPNET_ERR_ARG, "surface_spacing_tally: tau2 is NaN (a squared tolerance, or a negative value for none)");

    const hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)D * H * W;
    sps_u64* head = static_cast<sps_u64*>(workspace);
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + kSpsHeadBytes);
    double* gA = reinterpret_cast<double*>(static_cast<char*>(workspace) + kSpsHeadBytes + kSpsPartBytes);
    double* gB = gA + n;

    hipLaunchKernelGGL(surface_spacing_clear_kernel, dim3(cdiv(kSpsHeadWords, 256)), dim3(256), 0, st, head);

    SurfPair src{};
    src.p[0] = pred, src.p[1] = truth, src.kind[0] = pred_kind, src.kind[1] = truth_kind;
    surface_launch_passes(src, cls, D, H, W, SpsMetric{w[2]}, SpsMetric{w[1]}, SpsMetric{w[0]}, gA, gB, st);      // x, y, z: the tensor is [D, H, W]

    const int blocks = (int)std::min<size_t>((n + 255) / 256, (size_t)kSpsBlocks);
    const int iters = (int)((n + (size_t)blocks * 256 - 1) / ((size_t)blocks * 256));
    hipLaunchKernelGGL(surface_spacing_stats_kernel, dim3(blocks), dim3(256), 0, st, gA, gB, n, iters, tau2, head, part);
    for (int p = 0; p < kSpsPasses; ++p)
        hipLaunchKernelGGL(surface_spacing_radix_kernel, dim3(blocks), dim3(256), 0, st, gA, gB, n, iters, p, head);
    hipLaunchKernelGGL(surface_spacing_finalize_kernel, dim3(1), dim3(256), 0, st, head, part, blocks, (blocks + 255) / 256,
                       reinterpret_cast<long long*>(itable) + irow * RPNET_SURFACE_SPACING_IROW, ftable + frow * RPNET_SURFACE_SPACING_FROW);
    return check_launch("surface_spacing_tally");
}
