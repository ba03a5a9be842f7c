// The distance-transform core surface.hip (squared voxel distances in int32) and surface_spacing.hip (weighted squared distances in
// fp64) share: the border of either volume (foreground with a background 6-neighbour, outside = background) fused into the x pass, the
// separable min-plus transform out[i] = min_j (in[j] + cost(i - j)) along y and z, the checks of the arguments the two tallies have in
// common and the launches of the three passes.  Both volumes go through every pass in the same launch (a grid dimension of 2).
//
// A metric M is a small struct, passed to the kernels by value:
//   T                           the stored type
//   kNoSeed                     the transform of a line without a border voxel; kNoSeed + cost never comes out below kNoSeed
//   cost(o)                     of an offset of o voxels along the axis of the pass (the metric carries that axis' weight, if it has one)
//   add(a, b), lower(a, b)      the sum and the minimum, each one rounding at most
//   kTileBytes, kMaxTile, kMinTile   LDS of a y / z tile, its x columns at most, and the columns it keeps even when that takes more LDS
// Every operation is the metric's own, in the order written here: lower neighbour, then upper; the early stop is cost(o) >= best.
#ifndef RPNET_SURFACE_EDT_H
#define RPNET_SURFACE_EDT_H

#include "volume_kinds.h"

namespace rpnet {

constexpr int kSurfLineElems = RPNET_SURFACE_MAX_DIM;   // voxels a block of the x pass stages (whole lines)

struct SurfPair { const void* p[2]; int kind[2]; };

// x pass with the border fused in.  A block owns R = 1024 / W whole lines (line = z * H + y); grid (ceil(D*H / R), 2 volumes).
template <class M>
__global__ __launch_bounds__(256) void surface_x_kernel(const SurfPair src, const int cls, const int D, const int H, const int W, const int R,
                                                        const FastDiv div_w, const FastDiv div_h, const M m, typename M::T* __restrict__ gA,
                                                        typename M::T* __restrict__ gB) {
    RPNET_PASS_PRIORITY();
    __shared__ uint8_t fl[kSurfLineElems];      // bit 0: foreground; bit 1: the four y / z neighbours are foreground too
    __shared__ uint8_t bd[kSurfLineElems];      // border flag
    const int t = threadIdx.x, v = blockIdx.y;
    const void* __restrict__ p = src.p[v];
    const int kind = src.kind[v];
    typename M::T* __restrict__ g = v ? gB : gA;
    const int lines = D * H, line0 = blockIdx.x * R;
    const int cnt = min(R, lines - line0) * W;      // <= 1024
    const size_t HW = (size_t)H * W;

    for (int i = t; i < cnt; i += 256) {
        unsigned l, z;
        const int x = (int)div_w.divmod((unsigned)i, l);
        const int y = (int)div_h.divmod((unsigned)line0 + l, z);
        const size_t off = (size_t)(line0 + (int)l) * W + x;
        const bool f = vol_fg(p, kind, off, cls);
        const bool inner = f && y > 0 && y < H - 1 && z > 0 && (int)z < D - 1 && vol_fg(p, kind, off - W, cls) &&
                           vol_fg(p, kind, off + W, cls) && vol_fg(p, kind, off - HW, cls) && vol_fg(p, kind, off + HW, cls);
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
        typename M::T best = M::kNoSeed;
        for (int o = 0; o < W; ++o) {               // the first hit going outward is the nearest
            if ((x >= o && bd[i - o]) || (x + o < W && bd[i + o])) {
                best = m.cost(o);
                break;
            }
        }
        g[(size_t)line0 * W + i] = best;
    }
}

// y / z pass, in place.  A line has L voxels `lstride` apart; a block owns the lines of TX = 1 << txl neighbouring x columns of one
// outer index (y pass: outer = z, z pass: outer = y); grid (ceil(W / TX), n_outer, 2 volumes); LDS: L * TX values, all of it dynamic.
template <class M>
__global__ __launch_bounds__(256) void surface_line_kernel(typename M::T* __restrict__ gA, typename M::T* __restrict__ gB, const int L,
                                                           const size_t lstride, const size_t ostride, const int W, const int txl, const M m) {
    typedef typename M::T T;
    RPNET_PASS_PRIORITY();
    extern __shared__ __align__(16) unsigned char surface_tile[];
    T* __restrict__ s = reinterpret_cast<T*>(surface_tile);
    const int t = threadIdx.x, TX = 1 << txl, x0 = blockIdx.x << txl;
    const int nx = min(TX, W - x0), cnt = L << txl;                 // cnt * sizeof(T) is the LDS the launch asked for
    T* __restrict__ g = (blockIdx.z ? gB : gA) + (size_t)blockIdx.y * ostride + x0;

    for (int i = t; i < cnt; i += 256) {
        const int xl = i & (TX - 1), j = i >> txl;
        s[i] = xl < nx ? g[(size_t)j * lstride + xl] : M::kNoSeed;
    }
    __syncthreads();
    for (int i = t; i < cnt; i += 256) {
        const int xl = i & (TX - 1), j = i >> txl;
        if (xl >= nx) continue;
        T best = s[i];
        for (int o = 1; o < L; ++o) {
            const T c = m.cost(o);
            if (c >= best) break;                   // in[j] >= 0 and the cost grows with o: every further candidate is at least c
            if (j >= o) best = M::lower(best, M::add(s[i - (o << txl)], c));
            if (j + o < L) best = M::lower(best, M::add(s[i + (o << txl)], c));
        }
        g[(size_t)j * lstride + xl] = best;         // <= kNoSeed: it started there or below
    }
}

// The refusals the two tallies share, under the entry point's name `fn`; 0 when there is none.  need_of: the entry point's own
// workspace query, asked once the extents have passed.
static inline int surface_check_tally(const char* fn, const void* pred, int pred_kind, const void* truth, int truth_kind, int D, int H, int W,
                                      const void* itable, int64_t irow, const void* ftable, int64_t frow, int64_t n_rows, const void* workspace,
                                      size_t workspace_bytes, size_t (*need_of)(int, int, int)) {
    RPNET_REQUIRE(pred && truth && itable && ftable && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(pred_kind >= RPNET_SURFACE_U8 && pred_kind <= RPNET_SURFACE_F32 && truth_kind >= RPNET_SURFACE_U8 &&
                      truth_kind <= RPNET_SURFACE_F32,
                  RPNET_ERR_ARG, "%s: element kinds %d, %d (0 uint8, 1 int32, 2 int64, 3 float32)", fn, pred_kind, truth_kind);
    RPNET_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= RPNET_SURFACE_MAX_DIM && H <= RPNET_SURFACE_MAX_DIM && W <= RPNET_SURFACE_MAX_DIM,
                  RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_SURFACE_MAX_DIM);
    RPNET_REQUIRE(n_rows >= 1 && irow >= 0 && irow < n_rows && frow >= 0 && frow < n_rows, RPNET_ERR_ARG,
                  "%s: rows %lld and %lld of tables of %lld rows", fn, (long long)irow, (long long)frow, (long long)n_rows);
    const size_t need = need_of(D, H, W);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    static const size_t kAlign[4] = {1, 4, 8, 4};
    RPNET_REQUIRE(((uintptr_t)pred % kAlign[pred_kind]) == 0 && ((uintptr_t)truth % kAlign[truth_kind]) == 0 && ((uintptr_t)itable % 8) == 0 &&
                      ((uintptr_t)ftable % 8) == 0 && ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: volumes must be aligned to their element, the tables to 8 and the workspace to 16 bytes", fn);
    return 0;
}

// The x, y and z passes of both volumes on `st`; mx, my, mz: the metric of each axis.  A y / z tile is the widest power of two of
// columns up to kMaxTile that keeps the tile within kTileBytes, but not below kMinTile, and no wider than W needs.
template <class M>
static inline void surface_launch_passes(const SurfPair& src, int cls, int D, int H, int W, const M mx, const M my, const M mz,
                                         typename M::T* gA, typename M::T* gB, hipStream_t st) {
    const int R = kSurfLineElems / W, lines = D * H;
    hipLaunchKernelGGL(surface_x_kernel<M>, dim3(cdiv(lines, R), 2), dim3(256), 0, st, src, cls, D, H, W, R, FastDiv((unsigned)W),
                       FastDiv((unsigned)H), mx, gA, gB);
    // y pass: lines along H (stride W) per z; z pass: lines along D (stride H*W) per y
    const int len[2] = {H, D}, outer[2] = {D, H};
    const size_t lstride[2] = {(size_t)W, (size_t)H * W}, ostride[2] = {(size_t)H * W, (size_t)W};
    const M ml[2] = {my, mz};
    for (int a = 0; a < 2; ++a) {
        if (len[a] == 1) continue;                  // out[0] = in[0]
        int txl = 0;
        while ((2 << txl) <= M::kMaxTile && (1 << txl) < W &&
               ((size_t)len[a] * (2 << txl) * sizeof(typename M::T) <= (size_t)M::kTileBytes || (2 << txl) <= M::kMinTile))
            ++txl;
        const size_t lds = (size_t)len[a] * sizeof(typename M::T) << txl;       // <= 64 KiB: what a launch gets without asking
        hipLaunchKernelGGL(surface_line_kernel<M>, dim3(cdiv(W, 1 << txl), outer[a], 2), dim3(256), lds, st, gA, gB, len[a], lstride[a],
                           ostride[a], W, txl, ml[a]);
    }
}

}  // namespace rpnet
#endif  // RPNET_SURFACE_EDT_H
