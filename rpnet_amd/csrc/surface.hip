// Surface distances of an evaluated volume on the device (include/rpnet_surface_abi.h; rpnet_amd/surface.py): the tallies behind
// HD95, HD and ASSD of one prediction against one truth for one class.  With unit spacing every squared distance between voxels is an
// integer below D^2 + H^2 + W^2, so the device side is exact: the border of either volume (foreground with a background 6-neighbour,
// outside = background), the separable min-plus transform out[i] = min_j (in[j] + (i - j)^2) along x, y and z in int32 (the squared
// Euclidean distance to the nearest border voxel: Felzenszwalb & Huttenlocher 2012 state the decomposition; the lines here are short
// enough that the plain outward scan with its early stop beats the lower-envelope bookkeeping), a histogram over the squared distance
// with 64-bit integer counters, and one block that reads the order statistics and the two sums of square roots out of it.
//
// Launches of a tally: memset (histogram), x pass, y pass, z pass, histogram, finalize.  Both volumes go through every pass in the
// same launch (a grid dimension of 2).  The y and z passes are the hot part: a block owns the whole lines of a tile of neighbouring x
// columns, loads them row by row (coalesced) into LDS and writes the result back in place, so the two int32 volumes of the workspace
// are all the transform needs.  Bounds: every loop below runs to a count that is fixed when the loop is entered (line length, tile
// size, bins per thread); no thread waits on another block; blocks share nothing but integer atomicAdd on the histogram.
#include <algorithm>

#include "common.h"
#include "rpnet_surface_abi.h"

namespace rpnet {

constexpr int kSurfNoSeed = 1 << 29;                    // + 3 * 1024^2 < 2^31
constexpr int kSurfLineElems = RPNET_SURFACE_MAX_DIM;   // voxels a block of the x pass stages (whole lines)
constexpr int kSurfTileBytes = 32 * 1024;               // LDS of a y / z tile: 5 blocks per CU beside each other
constexpr int kSurfMaxTile = 64;                        // x columns per tile at most (a wave's worth of 4-byte columns)
constexpr int kSurfLocalBins = 1024;                    // bins a histogram block gathers in LDS (d < 32 voxels: nearly all of a good mask)
constexpr int kSurfHistBlocks = 2048;
static_assert(kSurfNoSeed + 3ll * RPNET_SURFACE_MAX_DIM * RPNET_SURFACE_MAX_DIM < (1ll << 31), "no seed + L^2 must fit int32");

struct SurfPair { const void* p[2]; int kind[2]; };

__device__ __forceinline__ bool surf_fg(const void* __restrict__ p, const int kind, const size_t i, const int cls) {
    switch (kind) {
        case RPNET_SURFACE_U8: return (int)static_cast<const uint8_t*>(p)[i] == cls;
        case RPNET_SURFACE_I32: return static_cast<const int32_t*>(p)[i] == cls;
        case RPNET_SURFACE_I64: return static_cast<const int64_t*>(p)[i] == (int64_t)cls;
        default: return static_cast<const float*>(p)[i] == (float)cls;
    }
}

// x pass with the border fused in.  A block owns R = 1024 / W whole lines (line = z * H + y); grid (ceil(D*H / R), 2 volumes).
__global__ __launch_bounds__(256) void surface_x_kernel(const SurfPair src, const int cls, const int D, const int H, const int W, const int R,
                                                        const FastDiv div_w, const FastDiv div_h, int32_t* __restrict__ gA,
                                                        int32_t* __restrict__ gB) {
    RPNET_PASS_PRIORITY();
    __shared__ uint8_t fl[kSurfLineElems];      // bit 0: foreground; bit 1: the four y / z neighbours are foreground too
    __shared__ uint8_t bd[kSurfLineElems];      // border flag
    const int t = threadIdx.x, v = blockIdx.y;
    const void* __restrict__ p = src.p[v];
    const int kind = src.kind[v];
    int32_t* __restrict__ g = v ? gB : gA;
    const int lines = D * H, line0 = blockIdx.x * R;
    const int cnt = min(R, lines - line0) * W;      // <= 1024
    const size_t HW = (size_t)H * W;

    for (int i = t; i < cnt; i += 256) {
        unsigned l, z;
        const int x = (int)div_w.divmod((unsigned)i, l);
        const int y = (int)div_h.divmod((unsigned)line0 + l, z);
        const size_t off = (size_t)(line0 + (int)l) * W + x;
        const bool f = surf_fg(p, kind, off, cls);
        const bool inner = f && y > 0 && y < H - 1 && z > 0 && (int)z < D - 1 && surf_fg(p, kind, off - W, cls) &&
                           surf_fg(p, kind, off + W, cls) && surf_fg(p, kind, off - HW, cls) && surf_fg(p, kind, off + HW, cls);
        fl[i] = (uint8_t)((f ? 1 : 0) | (inner ? 2 : 0));
    }
    __syncthreads();
    for (int i = t; i < cnt; i += 256) {
        const int x = (int)div_w.mod((unsigned)i);
        const unsigned c = fl[i];
        const bool eroded = (c & 2u) && x > 0 && x < W - 1 && (fl[i - 1] & 1u) && (fl[i + 1] & 1u);
        bd[i] = (uint8_t)((c & 1u) && !eroded);
    }
    __syncthreads();
    for (int i = t; i < cnt; i += 256) {
        const int x = (int)div_w.mod((unsigned)i);
        int best = kSurfNoSeed;
        for (int o = 0; o < W; ++o) {               // the first hit going outward is the nearest
            if ((x >= o && bd[i - o]) || (x + o < W && bd[i + o])) {
                best = o * o;
                break;
            }
        }
        g[(size_t)line0 * W + i] = best;
    }
}

// y / z pass, in place.  A line has L voxels `lstride` apart; a block owns the lines of TX = 1 << txl neighbouring x columns of one
// outer index (y pass: outer = z, z pass: outer = y); grid (ceil(W / TX), n_outer, 2 volumes); LDS: L * TX int32.
__global__ __launch_bounds__(256) void surface_line_kernel(int32_t* __restrict__ gA, int32_t* __restrict__ gB, const int L, const size_t lstride,
                                                           const size_t ostride, const int W, const int txl) {
    RPNET_PASS_PRIORITY();
    extern __shared__ int32_t s[];
    const int t = threadIdx.x, TX = 1 << txl, x0 = blockIdx.x << txl;
    const int nx = min(TX, W - x0), cnt = L << txl;                 // cnt * 4 <= kSurfTileBytes
    int32_t* __restrict__ g = (blockIdx.z ? gB : gA) + (size_t)blockIdx.y * ostride + x0;

    for (int i = t; i < cnt; i += 256) {
        const int xl = i & (TX - 1), j = i >> txl;
        s[i] = xl < nx ? g[(size_t)j * lstride + xl] : kSurfNoSeed;
    }
    __syncthreads();
    for (int i = t; i < cnt; i += 256) {
        const int xl = i & (TX - 1), j = i >> txl;
        if (xl >= nx) continue;
        int best = s[i];
        for (int o = 1; o < L; ++o) {
            const int o2 = o * o;
            if (o2 >= best) break;                  // every further candidate is at least o2
            if (j >= o) best = min(best, s[i - (o << txl)] + o2);
            if (j + o < L) best = min(best, s[i + (o << txl)] + o2);
        }
        g[(size_t)j * lstride + xl] = best;         // <= kSurfNoSeed: it started there or below
    }
}

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
    RPNET_REQUIRE(pred && truth && itable && ftable && workspace, RPNET_ERR_ARG, "surface_tally: null pointer");
    RPNET_REQUIRE(pred_kind >= RPNET_SURFACE_U8 && pred_kind <= RPNET_SURFACE_F32 && truth_kind >= RPNET_SURFACE_U8 &&
                      truth_kind <= RPNET_SURFACE_F32,
                  RPNET_ERR_ARG, "surface_tally: element kinds %d, %d (0 uint8, 1 int32, 2 int64, 3 float32)", pred_kind, truth_kind);
    RPNET_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= RPNET_SURFACE_MAX_DIM && H <= RPNET_SURFACE_MAX_DIM && W <= RPNET_SURFACE_MAX_DIM,
                  RPNET_ERR_SHAPE, "surface_tally: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_SURFACE_MAX_DIM);
    RPNET_REQUIRE(n_rows >= 1 && irow >= 0 && irow < n_rows && frow >= 0 && frow < n_rows, RPNET_ERR_ARG,
                  "surface_tally: rows %lld and %lld of tables of %lld rows", (long long)irow, (long long)frow, (long long)n_rows);
    const size_t need = rpnet_surface_workspace_bytes(D, H, W);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "surface_tally: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    static const size_t kAlign[4] = {1, 4, 8, 4};
    RPNET_REQUIRE(((uintptr_t)pred % kAlign[pred_kind]) == 0 && ((uintptr_t)truth % kAlign[truth_kind]) == 0 && ((uintptr_t)itable % 8) == 0 &&
                      ((uintptr_t)ftable % 8) == 0 && ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "surface_tally: volumes must be aligned to their element, the tables to 8 and the workspace to 16 bytes");

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
    const int R = kSurfLineElems / W, lines = D * H;
    hipLaunchKernelGGL(surface_x_kernel, dim3(cdiv(lines, R), 2), dim3(256), 0, st, src, cls, D, H, W, R, FastDiv((unsigned)W),
                       FastDiv((unsigned)H), gA, gB);

    // y pass: lines along H (stride W) per z; z pass: lines along D (stride H*W) per y
    const int len[2] = {H, D}, outer[2] = {D, H};
    const size_t lstride[2] = {(size_t)W, (size_t)H * W}, ostride[2] = {(size_t)H * W, (size_t)W};
    for (int a = 0; a < 2; ++a) {
        if (len[a] == 1) continue;                  // out[0] = in[0]
        int txl = 0;
        while ((2 << txl) <= kSurfMaxTile && (size_t)len[a] * (2 << txl) * sizeof(int32_t) <= (size_t)kSurfTileBytes && (1 << txl) < W) ++txl;
        const size_t lds = (size_t)len[a] * sizeof(int32_t) << txl;     // <= 32 KiB: L <= 1024 at txl = 0 is 4 KiB
        hipLaunchKernelGGL(surface_line_kernel, dim3(cdiv(W, 1 << txl), outer[a], 2), dim3(256), lds, st, gA, gB, len[a], lstride[a],
                           ostride[a], W, txl);
    }

    const int hblocks = (int)std::min<size_t>((n + 255) / 256, (size_t)kSurfHistBlocks);
    const int iters = (int)((n + (size_t)hblocks * 256 - 1) / ((size_t)hblocks * 256));
    hipLaunchKernelGGL(surface_hist_kernel, dim3(hblocks), dim3(256), 0, st, gA, gB, n, iters, nbins, hist, cnt);
    const long long per = (nbins + 255) / 256;
    hipLaunchKernelGGL(surface_finalize_kernel, dim3(1), dim3(256), 0, st, hist, cnt, nbins, per,
                       reinterpret_cast<long long*>(itable) + irow * RPNET_SURFACE_IROW, ftable + frow * RPNET_SURFACE_FROW);
    return check_launch("surface_tally");
}
