// Surface distances of an evaluated volume on the device (include/rpnet_surface_abi.h; rpnet_amd/surface.py): the tallies behind
// HD95, HD and ASSD of one prediction against one truth for one class.  With unit spacing every squared distance between voxels is an
// integer below D^2 + H^2 + W^2, so the device side is exact: the border of either volume (foreground with a background 6-neighbour,
// outside = background), the separable min-plus transform out[i] = min_j (in[j] + (i - j)^2) along x, y and z in int32 (the squared
// Euclidean distance to the nearest border voxel: Felzenszwalb & Huttenlocher 2012 state the decomposition; the lines here are short
// enough that the plain outward scan with its early stop beats the lower-envelope bookkeeping), a histogram over the squared distance
// with 64-bit integer counters, and one block that reads the order statistics and the two sums of square roots out of it.
//
// Launches of a tally: memset (histogram), x pass, y pass, z pass, histogram, finalize.  Both volumes go through every pass in the
// same launch (a grid dimension of 2).  The three passes are the kernels of surface_edt.h under the integer metric below; the y and z
// passes are the hot part: a block owns the whole lines of a tile of neighbouring x
// columns, loads them row by row (coalesced) into LDS and writes the result back in place, so the two int32 volumes of the workspace
// are all the transform needs.  Bounds: every loop below runs to a count that is fixed when the loop is entered (line length, tile
// size, bins per thread); no thread waits on another block; blocks share nothing but integer atomicAdd on the histogram.
#include <algorithm>

#include "surface_edt.h"

namespace rpnet {

constexpr int kSurfLocalBins = 1024;                    // bins a histogram block gathers in LDS (d < 32 voxels: nearly all of a good mask)
constexpr int kSurfHistBlocks = 2048;

struct SurfMetric {                                     // squared voxel distances: every value an integer below D^2 + H^2 + W^2
    typedef int32_t T;
    static constexpr T kNoSeed = 1 << 29;               // + 3 * 1024^2 < 2^31
    static constexpr int kTileBytes = 32 * 1024;        // LDS of a y / z tile: 5 blocks per CU beside each other
    static constexpr int kMaxTile = 64, kMinTile = 1;   // x columns per tile at most (a wave's worth of 4-byte columns); no floor
    __device__ __forceinline__ T cost(const int o) const { return o * o; }
    static __device__ __forceinline__ T add(const T a, const T b) { return a + b; }
    static __device__ __forceinline__ T lower(const T a, const T b) { return min(a, b); }
};
static_assert(SurfMetric::kNoSeed + 3ll * RPNET_SURFACE_MAX_DIM * RPNET_SURFACE_MAX_DIM < (1ll << 31), "no seed + L^2 must fit int32");

// hist[0][d2 to border(B)] += 1 for the voxels of border(A), hist[1][d2 to border(A)] += 1 for those of border(B); cnt = {n_A, n_B}.
// A voxel is on a border exactly where that volume's transform is 0.  `iters` grid-sized sweeps cover the n voxels.
__global__ __launch_bounds__(256) void surface_hist_kernel(const int32_t* __restrict__ gA, const int32_t* __restrict__ gB, const size_t n,
                                                           const int iters, const long long nbins, unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ cnt) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned lh[2 * kSurfLocalBins];
    __shared__ unsigned lc[2];
    const int t = threadIdx.x;
    for (int j = t; j < 2 * kSurfLocalBins; j += 256) lh[j] = 0u;
    if (t < 2) lc[t] = 0u;
    __syncthreads();
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)it * gridDim.x + blockIdx.x) * 256u + t;
        int a = 1, b = 1;
        if (i < n) {
            a = gA[i];
            b = gB[i];
        }
        if (a == 0) {
            atomicAdd(&lc[0], 1u);
            if (b < kSurfLocalBins) atomicAdd(&lh[b], 1u);
            else if (b < nbins) atomicAdd(hist + b, 1ull);
        }
        if (b == 0) {
            atomicAdd(&lc[1], 1u);
            if (a < kSurfLocalBins) atomicAdd(&lh[kSurfLocalBins + a], 1u);
            else if (a < nbins) atomicAdd(hist + nbins + a, 1ull);
        }
    }
    __syncthreads();
    for (int j = t; j < 2 * kSurfLocalBins; j += 256) {
        const unsigned c = lh[j];
        const int h = j >= kSurfLocalBins ? 1 : 0, bin = j - h * kSurfLocalBins;
        if (c && bin < nbins) atomicAdd(hist + (size_t)h * nbins + bin, (unsigned long long)c);
    }
    if (t < 2 && lc[t]) atomicAdd(cnt + t, (unsigned long long)lc[t]);
}

// One block.  Thread t owns the bins [t * per, (t + 1) * per): pooled count, largest used bin and the two sums of count * sqrt(bin)
// in bin order; the 256 partial results are combined in thread order by thread 0, which also finds the threads that hold the ranks k
// and k1; those rescan their bins for the rank.
__global__ __launch_bounds__(256) void surface_finalize_kernel(const unsigned long long* __restrict__ hist,
                                                               const unsigned long long* __restrict__ cnt, const long long nbins,
                                                               const long long per, long long* __restrict__ irow, double* __restrict__ frow) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned long long pc[256];
    __shared__ long long pmax[256];
    __shared__ double pf[2][256];
    __shared__ long long want[2], owner[2];
    __shared__ unsigned long long before[2];
    const int t = threadIdx.x;
    const unsigned long long nA = cnt[0], nB = cnt[1];
    if (nA == 0 || nB == 0) {                                       // block-uniform
        if (t < RPNET_SURFACE_IROW) irow[t] = t == RPNET_SURFACE_IROW - 1 ? -1 : 0;
        if (t < RPNET_SURFACE_FROW) frow[t] = 0.0;
        return;
    }
    const long long lo = min((long long)t * per, nbins), hi = min(lo + per, nbins);
    unsigned long long c = 0;
    long long mx = -1;
    double fa = 0.0, fb = 0.0;
    for (long long b = lo; b < hi; ++b) {
        const unsigned long long ca = hist[b], cb = hist[nbins + b];
        if (ca | cb) {
            const double r = sqrt((double)b);
            fa += (double)ca * r;
            fb += (double)cb * r;
            c += ca + cb;
            mx = b;
        }
    }
    pc[t] = c;
    pmax[t] = mx;
    pf[0][t] = fa;
    pf[1][t] = fb;
    __syncthreads();
    if (t == 0) {
        const unsigned long long n = nA + nB;
        const long long k = (long long)floor(0.95 * (double)(n - 1));      // numpy: virtual index (n - 1) * (95 / 100), then floor
        want[0] = k;
        want[1] = min(k + 1, (long long)n - 1);
        owner[0] = owner[1] = -1;
        unsigned long long run = 0;
        long long dmax = 0;
        double sa = 0.0, sb = 0.0;
        for (int j = 0; j < 256; ++j) {
            for (int q = 0; q < 2; ++q)
                if (owner[q] < 0 && run + pc[j] > (unsigned long long)want[q]) {
                    owner[q] = j;
                    before[q] = run;
                }
            run += pc[j];
            dmax = max(dmax, pmax[j]);
            sa += pf[0][j];
            sb += pf[1][j];
        }
        irow[0] = (long long)nA;
        irow[1] = (long long)nB;
        irow[4] = dmax;
        irow[5] = k;
        frow[0] = sa;
        frow[1] = sb;
    }
    __syncthreads();
    for (int q = 0; q < 2; ++q) {
        if (owner[q] != t) continue;
        unsigned long long run = before[q];
        long long found = 0;
        for (long long b = lo; b < hi; ++b) {
            run += hist[b] + hist[nbins + b];
            if (run > (unsigned long long)want[q]) {
                found = b;
                break;
            }
        }
        irow[2 + q] = found;
    }
}

static inline long long surf_nbins(int D, int H, int W) {
    return (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) + 1;
}
static inline size_t surf_hist_bytes(int D, int H, int W) {            // the two histograms and {n_A, n_B}, a multiple of 16
    return ((size_t)(2 * surf_nbins(D, H, W) + 2) * 8 + 15) / 16 * 16;
}

}  // namespace rpnet

extern "C" int rpnet_surface_abi_version(void) { return RPNET_SURFACE_ABI_VERSION; }

extern "C" size_t rpnet_surface_workspace_bytes(int D, int H, int W) {
    using namespace rpnet;
    if (D < 1 || H < 1 || W < 1 || D > RPNET_SURFACE_MAX_DIM || H > RPNET_SURFACE_MAX_DIM || W > RPNET_SURFACE_MAX_DIM) {
        set_error("surface: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_SURFACE_MAX_DIM);
        return 0;
    }
    return surf_hist_bytes(D, H, W) + 2 * (size_t)D * H * W * sizeof(int32_t);
}

extern "C" int rpnet_surface_tally(const void* pred, int pred_kind, const void* truth, int truth_kind, int cls, int D, int H, int W,
                                   int64_t* itable, int64_t irow, double* ftable, int64_t frow, int64_t n_rows, void* workspace,
                                   size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    if (const int rc = surface_check_tally("surface_tally", pred, pred_kind, truth, truth_kind, D, H, W, itable, irow, ftable, frow, n_rows,
                                           workspace, workspace_bytes, rpnet_surface_workspace_bytes))
        return rc;

    const hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)D * H * W, hist_bytes = surf_hist_bytes(D, H, W);
    const long long nbins = surf_nbins(D, H, W);
    unsigned long long* hist = static_cast<unsigned long long*>(workspace);
    unsigned long long* cnt = hist + 2 * nbins;
    int32_t* gA = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + hist_bytes);
    int32_t* gB = gA + n;

    if (hipMemsetAsync(workspace, 0, hist_bytes, st) != hipSuccess) {
        const int rc = check_launch("surface_tally (memset)");
        return rc ? rc : RPNET_ERR_ARG;
    }

    SurfPair src{};
    src.p[0] = pred, src.p[1] = truth, src.kind[0] = pred_kind, src.kind[1] = truth_kind;
    surface_launch_passes(src, cls, D, H, W, SurfMetric{}, SurfMetric{}, SurfMetric{}, gA, gB, st);

    const int hblocks = (int)std::min<size_t>((n + 255) / 256, (size_t)kSurfHistBlocks);
    const int iters = (int)((n + (size_t)hblocks * 256 - 1) / ((size_t)hblocks * 256));
    hipLaunchKernelGGL(surface_hist_kernel, dim3(hblocks), dim3(256), 0, st, gA, gB, n, iters, nbins, hist, cnt);
    const long long per = (nbins + 255) / 256;
    hipLaunchKernelGGL(surface_finalize_kernel, dim3(1), dim3(256), 0, st, hist, cnt, nbins, per,
                       reinterpret_cast<long long*>(itable) + irow * RPNET_SURFACE_IROW, ftable + frow * RPNET_SURFACE_FROW);
    return check_launch("surface_tally");
}
