// Ball morphology of one class of a segmented volume on the device: erode, dilate, open, close (include/rpnet_morph_abi.h;
// rpnet_amd/morphology.py).  A ball is the one structuring element for which the separable distance transform of surface_edt.h gives
// morphology exactly: dilate(X) = {v : d2(v, X) <= rho}, erode(X) = {v : d2(v, Omega \ X) > rho}.  This file is the third customer of
// that transform: its y / z line pass is the one of surface_line_kernel (lines staged in LDS, lower neighbour, then upper, the early
// stop cost(o) >= best) with two additions that the tallies cannot use, so it is instantiated here and the two tallies stay as they are:
//   the cap      only `<= rho` is ever asked of a value, so every value above rho is stored as the first value above it (rho + 1;
//                nextafter(r2) in fp64).  best starts at min(in, cap) and the early stop then ends every scan at the ball's extent along
//                the axis, whatever the line holds: a pass costs O(ball radius) per voxel instead of O(distance to the nearest seed);
//   the result   the last pass of a transform writes the uint8 set, not distances.
// The x pass is new: the seeds are the object (dilation) or its complement (erosion), read from the volume of any element kind or from
// the uint8 result of the first transform of an opening / closing.
//
// Metrics: squared voxel distances in int32 (MorphVox), weighted squared distances in fp64 with every product and every sum one
// rounding (MorphMm: the operations of SpsMetric in the order of its passes; the file is built with -ffp-contract=off).
//
// Launches of a call: per transform x, y, z (an axis of length 1 has no pass, per-slice mode no z pass; the first x pass clears the
// head), then write back + tally, then the statistics row.  Bounds: every loop runs to a count fixed when it is entered (the line
// length, the tile, the sweeps of a block, the 16 voxels of a lane); no thread waits on another block; blocks share nothing but integer
// atomics, one per counter and block.
#include <algorithm>
#include <cmath>

#include "rpnet_morph_abi.h"
#include "surface_edt.h"

namespace rpnet {

typedef unsigned long long morph_u64;

constexpr size_t kMorphHeadBytes = 64;              // 8 counters: before, after, added, removed (4 spare)
constexpr int kMorphLane = 16;                      // voxels of a lane in the write-back launch: one 16-byte store of out
constexpr int kMorphBlocks = 2048;                  // blocks of the write-back launch at most
static_assert(RPNET_CC_MAX_DIM == RPNET_SURFACE_MAX_DIM, "the x pass stages whole lines of kSurfLineElems voxels");
static_assert(RPNET_MORPH_MAX_RHO == 3ll * RPNET_CC_MAX_DIM * RPNET_CC_MAX_DIM, "the squared diagonal");

struct MorphVox {                                   // squared voxel distances, capped at rho + 1
    typedef int32_t T;
    T lim;                                          // rho
    static constexpr int kTileBytes = 32 * 1024;    // the LDS budget of SurfMetric
    static constexpr int kMaxTile = 64, kMinTile = 1;
    __host__ __device__ __forceinline__ T cap() const { return lim + 1; }
    __host__ __device__ __forceinline__ T cost(const int o) const { return o * o; }
    static __device__ __forceinline__ T add(const T a, const T b) { return a + b; }    // <= rho + 1 + 1023^2 < 2^31
    static __device__ __forceinline__ T lower(const T a, const T b) { return min(a, b); }
};

struct MorphMm {                                    // w * o^2 along one axis, capped at the double after r2
    typedef double T;
    double w, lim, capv;                            // the weight of the axis of the pass, r2, nextafter(r2, inf)
    static constexpr int kTileBytes = 32 * 1024;    // the LDS budget of SpsMetric: 64 KiB only for lines above 512
    static constexpr int kMaxTile = 32, kMinTile = 8;
    __host__ __device__ __forceinline__ T cap() const { return capv; }
    __host__ __device__ __forceinline__ T cost(const int o) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return __dmul_rn(w, (double)(o * o));
#else
        return w * (double)(o * o);                 // the host's product is one IEEE rounding too (morph_reach)
#endif
    }
    static __device__ __forceinline__ T add(const T a, const T b) { return __dadd_rn(a, b); }
    static __device__ __forceinline__ T lower(const T a, const T b) { return fmin(a, b); }
};
static_assert((size_t)RPNET_CC_MAX_DIM * MorphMm::kMinTile * sizeof(double) <= 64 * 1024, "the longest line, narrowest tile: 64 KiB");

// where the seeds of a transform come from: the voxels with (value == cls) != invert
struct MorphSeeds { const void* p; int kind, cls, invert; };
// the erode_border = 0 rule of the transform's result: a voxel fewer than o* voxels from a face of its axis is eroded (o*: the
// offsets o >= 1 of that axis with cost(o) <= rho, counted on the host; all 0: no rule).  erode: the result is `> rho`, else `<= rho`
struct MorphEdge { int erode, ox, oy, oz; };

template <class M>
__device__ __forceinline__ uint8_t morph_result(const typename M::T best, const M& m, const MorphEdge& e, const int x, const int y, const int z,
                                                const int D, const int H, const int W) {
    if (!e.erode) return (uint8_t)(best <= m.lim);
    const bool edge = x < e.ox || W - 1 - x < e.ox || y < e.oy || H - 1 - y < e.oy || z < e.oz || D - 1 - z < e.oz;
    return (uint8_t)(best > m.lim && !edge);
}

// Seeded x pass.  A block owns R = 1024 / W whole lines (line = z * H + y); grid ceil(D*H / R).  kLast: there is no y and no z pass,
// so the result is written.  head: cleared by block 0 when not null (the first launch of a call).
template <class M, bool kLast>
__global__ __launch_bounds__(256) void morph_x_kernel(const MorphSeeds src, const int D, const int H, const int W, const int R, const FastDiv div_w,
                                                      const FastDiv div_h, const M m, const MorphEdge edge, typename M::T* __restrict__ g,
                                                      uint8_t* __restrict__ res, morph_u64* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ uint8_t sd[kSurfLineElems];
    const int t = threadIdx.x;
    if (head && blockIdx.x == 0 && t < (int)(kMorphHeadBytes / sizeof(morph_u64))) head[t] = 0ull;
    const int lines = D * H, line0 = blockIdx.x * R;
    const int cnt = min(R, lines - line0) * W;      // <= 1024
    const size_t base = (size_t)line0 * W;
    for (int i = t; i < cnt; i += 256) sd[i] = (uint8_t)(vol_fg(src.p, src.kind, base + i, src.cls) != (src.invert != 0));
    __syncthreads();
    const typename M::T cap = m.cap();
    for (int i = t; i < cnt; i += 256) {
        unsigned l, z;
        const int x = (int)div_w.divmod((unsigned)i, l);
        typename M::T best = cap;
        for (int o = 0; o < W; ++o) {               // the first hit going outward is the nearest; beyond the ball nothing matters
            const typename M::T c = m.cost(o);
            if (c >= cap) break;
            if ((x >= o && sd[i - o]) || (x + o < W && sd[i + o])) {
                best = c;
                break;
            }
        }
        if (kLast) {
            const int y = (int)div_h.divmod((unsigned)line0 + l, z);
            res[base + i] = morph_result(best, m, edge, x, y, (int)z, D, H, W);
        } else {
            g[base + i] = best;
        }
    }
}

// y / z pass: surface_line_kernel with the cap, on one volume.  A line has L voxels `lstride` apart; a block owns the lines of
// TX = 1 << txl neighbouring x columns of one outer index (y pass: outer = z, z pass: outer = y); grid (ceil(W / TX), n_outer);
// LDS: L * TX values, all of it dynamic.  kLast: the result is written to res instead of the distances to g.  zpass: the line runs along z.
template <class M, bool kLast>
__global__ __launch_bounds__(256) void morph_line_kernel(typename M::T* __restrict__ gv, uint8_t* __restrict__ res, const int L, const size_t lstride,
                                                         const size_t ostride, const int D, const int H, const int W, const int txl, const int zpass,
                                                         const M m, const MorphEdge edge) {
    typedef typename M::T T;
    RPNET_PASS_PRIORITY();
    extern __shared__ __align__(16) unsigned char morph_tile[];
    T* __restrict__ s = reinterpret_cast<T*>(morph_tile);
    const int t = threadIdx.x, TX = 1 << txl, x0 = blockIdx.x << txl;
    const int nx = min(TX, W - x0), cnt = L << txl;                 // cnt * sizeof(T) is the LDS the launch asked for
    const size_t obase = (size_t)blockIdx.y * ostride + x0;
    T* __restrict__ g = gv + obase;
    const T cap = m.cap();

    for (int i = t; i < cnt; i += 256) {
        const int xl = i & (TX - 1), j = i >> txl;
        s[i] = xl < nx ? M::lower(g[(size_t)j * lstride + xl], cap) : cap;
    }
    __syncthreads();
    for (int i = t; i < cnt; i += 256) {
        const int xl = i & (TX - 1), j = i >> txl;
        if (xl >= nx) continue;
        T best = s[i];                              // <= cap
        for (int o = 1; o < L; ++o) {
            const T c = m.cost(o);
            if (c >= best) break;                   // in[j] >= 0 and the cost grows with o: every further candidate is at least c
            if (j >= o) best = M::lower(best, M::add(s[i - (o << txl)], c));
            if (j + o < L) best = M::lower(best, M::add(s[i + (o << txl)], c));
        }
        if (kLast) {
            const int y = zpass ? (int)blockIdx.y : j, z = zpass ? j : (int)blockIdx.y;
            res[obase + (size_t)j * lstride + xl] = morph_result(best, m, edge, x0 + xl, y, z, D, H, W);
        } else {
            g[(size_t)j * lstride + xl] = best;
        }
    }
}

// Write back and tally.  A lane owns kMorphLane consecutive voxels: it reads them, then writes them (one 16-byte store where `vec` says
// that out is 16-byte aligned and the lane's voxels are all inside the volume), and touches no other element of in or out, so the two
// may be one uint8 volume.  res: the set the operation gives.  The rule: a voxel of the class that the set lacks becomes 0; a voxel of
// value 0 that the set holds becomes cls; everything else passes through.
__global__ __launch_bounds__(256) void morph_apply_kernel(const void* in, const int kind, uint8_t* out, const int cls, const uint8_t* __restrict__ res,
                                                          const void* truth, const int truth_kind, morph_u64* __restrict__ counts, const size_t n,
                                                          const size_t n_lanes, const int iters, const int vec, morph_u64* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned sc[7];                      // before, after, added, removed, |P and T|, |P|, |T|
    const int t = threadIdx.x;
    if (t < 7) sc[t] = 0u;
    __syncthreads();
    unsigned before = 0u, after = 0u, added = 0u, removed = 0u, c_pt = 0u, c_t = 0u;
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)blockIdx.x * iters + it) * 256u + t;
        if (lane >= n_lanes) continue;
        const size_t base = lane * kMorphLane;
        const int cnt = (int)std::min<size_t>((size_t)kMorphLane, n - base);
        union {
            uint8_t b[kMorphLane];
            uint4 q;
        } o;
        uint8_t r[kMorphLane];
        if (cnt == kMorphLane) {                    // res starts 16-byte aligned inside the workspace
            const uint4 q = *reinterpret_cast<const uint4*>(res + base);
            __builtin_memcpy(r, &q, sizeof(q));
        } else {
#pragma unroll
            for (int j = 0; j < kMorphLane; ++j) r[j] = j < cnt ? res[base + j] : (uint8_t)0;
        }
#pragma unroll
        for (int j = 0; j < kMorphLane; ++j) {
            if (j >= cnt) continue;
            const size_t i = base + j;
            const uint8_t v = vol_u8(in, kind, i);
            const bool was = vol_fg(in, kind, i, cls), set = r[j] != 0;
            const bool gain = set && !was && vol_fg(in, kind, i, 0), loss = was && !set;
            const bool pred = (was && set) || gain;
            o.b[j] = gain ? (uint8_t)cls : (loss ? (uint8_t)0 : v);
            before += was;
            after += pred;
            added += gain;
            removed += loss;
            if (truth) {
                const bool tr = vol_fg(truth, truth_kind, i, cls);
                c_pt += pred && tr;
                c_t += tr;
            }
        }
        if (vec && cnt == kMorphLane) {
            *reinterpret_cast<uint4*>(out + base) = o.q;
        } else {
            for (int j = 0; j < cnt; ++j) out[base + j] = o.b[j];
        }
    }
    if (before) atomicAdd(&sc[0], before);
    if (after) atomicAdd(&sc[1], after);
    if (added) atomicAdd(&sc[2], added);
    if (removed) atomicAdd(&sc[3], removed);
    if (c_pt) atomicAdd(&sc[4], c_pt);
    if (truth && after) atomicAdd(&sc[5], after);
    if (c_t) atomicAdd(&sc[6], c_t);
    __syncthreads();
    if (t < 4 && sc[t]) atomicAdd(head + t, (morph_u64)sc[t]);
    if (t >= 4 && t < 7 && counts && sc[t]) atomicAdd(counts + (t - 4), (morph_u64)sc[t]);
}

__global__ __launch_bounds__(64) void morph_stats_kernel(const morph_u64* __restrict__ head, long long* __restrict__ row) {
    const int t = threadIdx.x;
    if (t < RPNET_MORPH_STATS_ROW) row[t] = (long long)head[t];
}

struct MorphArgs {
    const void* in;
    int kind_in;
    uint8_t* out;
    int cls, D, H, W, op, per_slice, erode_border;
    const void* truth;
    int truth_kind;
    int64_t *counts, counts_row, *stats, stats_row, n_rows;
    void* workspace;
    size_t workspace_bytes;
};

static inline bool morph_dims_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= RPNET_CC_MAX_DIM && H <= RPNET_CC_MAX_DIM && W <= RPNET_CC_MAX_DIM;
}
static inline size_t morph_up16(size_t b) { return (b + 15) / 16 * 16; }
static inline size_t morph_need(int D, int H, int W) {
    const size_t n = (size_t)D * H * W;
    return kMorphHeadBytes + morph_up16(n * 8) + 2 * morph_up16(n);
}

// the refusals the two entry points share; `fn` names the entry point in the message
static int morph_check(const char* fn, const MorphArgs& a) {
    static const size_t kElem[4] = {1, 4, 8, 4};
    RPNET_REQUIRE(a.in && a.out && a.stats && a.workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE((a.truth == nullptr) == (a.counts == nullptr), RPNET_ERR_ARG, "%s: truth and counts come together (both or neither)", fn);
    RPNET_REQUIRE(a.kind_in >= RPNET_CC_U8 && a.kind_in <= RPNET_CC_F32 && (!a.truth || (a.truth_kind >= RPNET_CC_U8 && a.truth_kind <= RPNET_CC_F32)),
                  RPNET_ERR_ARG, "%s: element kinds %d, %d (0 uint8, 1 int32, 2 int64, 3 float32)", fn, a.kind_in, a.truth_kind);
    RPNET_REQUIRE(a.op >= RPNET_MORPH_ERODE && a.op <= RPNET_MORPH_CLOSE, RPNET_ERR_ARG, "%s: op %d (0 erode, 1 dilate, 2 open, 3 close)", fn, a.op);
    RPNET_REQUIRE(a.cls >= 1 && a.cls <= 255, RPNET_ERR_ARG, "%s: class %d (1..255: the output is uint8)", fn, a.cls);
    RPNET_REQUIRE(morph_dims_ok(a.D, a.H, a.W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, a.D, a.H, a.W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(a.n_rows >= 1 && a.stats_row >= 0 && a.stats_row < a.n_rows && (!a.counts || (a.counts_row >= 0 && a.counts_row < a.n_rows)),
                  RPNET_ERR_ARG, "%s: rows %lld and %lld of tables of %lld rows", fn, (long long)a.counts_row, (long long)a.stats_row,
                  (long long)a.n_rows);
    const size_t need = morph_need(a.D, a.H, a.W);
    RPNET_REQUIRE(a.workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, a.workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)a.in % kElem[a.kind_in]) == 0 && (!a.truth || ((uintptr_t)a.truth % kElem[a.truth_kind]) == 0) &&
                      ((uintptr_t)a.stats % 8) == 0 && ((uintptr_t)a.counts % 8) == 0 && ((uintptr_t)a.workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: volumes must be aligned to their element, the tables to 8 and the workspace to 16 bytes", fn);
    const size_t n = (size_t)a.D * a.H * a.W;
    const uintptr_t a0 = (uintptr_t)a.in, a1 = a0 + n * kElem[a.kind_in], b0 = (uintptr_t)a.out, b1 = b0 + n;
    RPNET_REQUIRE((a.kind_in == RPNET_CC_U8 && a0 == b0) || a1 <= b0 || b1 <= a0, RPNET_ERR_ARG,
                  "%s: out overlaps in (only a uint8 volume can be processed in place, out == in)", fn);
    return 0;
}

// the offsets o in 1..L of an axis with cost(o) <= lim, on the host with the metric's own operations (the cost grows with o)
template <class M>
static int morph_reach(const M& m, const int L) {
    int o = 0;
    while (o < L && m.cost(o + 1) <= m.lim) ++o;
    return o;
}

// One transform: the seeds of `src` -> the uint8 set `res` (erode: `> rho` with the border rule, else `<= rho`).  g: the distances
// between the passes.  A y / z tile is chosen as surface_launch_passes chooses it.
template <class M>
static void morph_transform(const MorphSeeds& src, const bool erode, const MorphArgs& a, const M mx, const M my, const M mz,
                            typename M::T* g, uint8_t* res, morph_u64* head, hipStream_t st) {
    typedef typename M::T T;
    const int D = a.D, H = a.H, W = a.W;
    const bool ypass = H > 1, zpass = D > 1 && !a.per_slice;
    MorphEdge edge{erode ? 1 : 0, 0, 0, 0};
    if (erode && !a.erode_border) {
        edge.ox = morph_reach(mx, W);
        edge.oy = morph_reach(my, H);
        edge.oz = a.per_slice ? 0 : morph_reach(mz, D);
    }
    const int R = kSurfLineElems / W, lines = D * H;
    const FastDiv div_w((unsigned)W), div_h((unsigned)H);
    if (!ypass && !zpass)
        hipLaunchKernelGGL((morph_x_kernel<M, true>), dim3(cdiv(lines, R)), dim3(256), 0, st, src, D, H, W, R, div_w, div_h, mx, edge, g, res, head);
    else
        hipLaunchKernelGGL((morph_x_kernel<M, false>), dim3(cdiv(lines, R)), dim3(256), 0, st, src, D, H, W, R, div_w, div_h, mx, edge, g, res, head);
    // y pass: lines along H (stride W) per z; z pass: lines along D (stride H*W) per y
    const int len[2] = {H, D}, outer[2] = {D, H};
    const bool on[2] = {ypass, zpass};
    const size_t lstride[2] = {(size_t)W, (size_t)H * W}, ostride[2] = {(size_t)H * W, (size_t)W};
    const M ml[2] = {my, mz};
    for (int ax = 0; ax < 2; ++ax) {
        if (!on[ax]) continue;
        int txl = 0;
        while ((2 << txl) <= M::kMaxTile && (1 << txl) < W &&
               ((size_t)len[ax] * (2 << txl) * sizeof(T) <= (size_t)M::kTileBytes || (2 << txl) <= M::kMinTile))
            ++txl;
        const size_t lds = (size_t)len[ax] * sizeof(T) << txl;      // <= 64 KiB: what a launch gets without asking
        const dim3 grid(cdiv(W, 1 << txl), outer[ax]);
        const bool last = ax == 1 || !zpass;
        if (last)
            hipLaunchKernelGGL((morph_line_kernel<M, true>), grid, dim3(256), lds, st, g, res, len[ax], lstride[ax], ostride[ax], D, H, W, txl, ax, ml[ax],
                               edge);
        else
            hipLaunchKernelGGL((morph_line_kernel<M, false>), grid, dim3(256), lds, st, g, res, len[ax], lstride[ax], ostride[ax], D, H, W, txl, ax,
                               ml[ax], edge);
    }
}

// every argument has been checked
template <class M>
static int morph_run(const char* fn, const MorphArgs& a, const M mx, const M my, const M mz, hipStream_t st) {
    const size_t n = (size_t)a.D * a.H * a.W;
    char* ws = static_cast<char*>(a.workspace);
    morph_u64* head = reinterpret_cast<morph_u64*>(ws);
    typename M::T* g = reinterpret_cast<typename M::T*>(ws + kMorphHeadBytes);
    uint8_t* mid = reinterpret_cast<uint8_t*>(ws + kMorphHeadBytes + morph_up16(n * 8));
    uint8_t* res = mid + morph_up16(n);
    const MorphSeeds object{a.in, a.kind_in, a.cls, 0}, complement{a.in, a.kind_in, a.cls, 1};
    const MorphSeeds mid_object{mid, RPNET_CC_U8, 1, 0}, mid_complement{mid, RPNET_CC_U8, 1, 1};
    switch (a.op) {
        case RPNET_MORPH_ERODE: morph_transform(complement, true, a, mx, my, mz, g, res, head, st); break;
        case RPNET_MORPH_DILATE: morph_transform(object, false, a, mx, my, mz, g, res, head, st); break;
        case RPNET_MORPH_OPEN:
            morph_transform(complement, true, a, mx, my, mz, g, mid, head, st);
            morph_transform(mid_object, false, a, mx, my, mz, g, res, static_cast<morph_u64*>(nullptr), st);
            break;
        default:
            morph_transform(object, false, a, mx, my, mz, g, mid, head, st);
            morph_transform(mid_complement, true, a, mx, my, mz, g, res, static_cast<morph_u64*>(nullptr), st);
    }
    const size_t n_lanes = (n + kMorphLane - 1) / kMorphLane;
    const int blocks = (int)std::min<size_t>((n_lanes + 255) / 256, (size_t)kMorphBlocks);
    const int iters = (int)((n_lanes + (size_t)blocks * 256 - 1) / ((size_t)blocks * 256));
    hipLaunchKernelGGL(morph_apply_kernel, dim3(blocks), dim3(256), 0, st, a.in, a.kind_in, a.out, a.cls, res, a.truth, a.truth_kind,
                       a.counts ? reinterpret_cast<morph_u64*>(a.counts) + a.counts_row * RPNET_MORPH_COUNTS_ROW : nullptr, n, n_lanes, iters,
                       (int)(((uintptr_t)a.out % 16) == 0), head);
    hipLaunchKernelGGL(morph_stats_kernel, dim3(1), dim3(64), 0, st, head, reinterpret_cast<long long*>(a.stats) + a.stats_row * RPNET_MORPH_STATS_ROW);
    return check_launch(fn);
}

}  // namespace rpnet

extern "C" int rpnet_morph_abi_version(void) { return RPNET_MORPH_ABI_VERSION; }

extern "C" size_t rpnet_morph_workspace_bytes(int D, int H, int W) {
    using namespace rpnet;
    if (!morph_dims_ok(D, H, W)) {
        set_error("morph: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_CC_MAX_DIM);
        return 0;
    }
    return morph_need(D, H, W);
}

extern "C" int rpnet_morph_apply(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int op, int64_t rho, int per_slice,
                                 int erode_border, const void* truth, int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats,
                                 int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "morph_apply";
    const MorphArgs a{in,     kind_in,    out,   cls,       D,      H,         W,         op, per_slice != 0, erode_border != 0, truth, truth_kind,
                      counts, counts_row, stats, stats_row, n_rows, workspace, workspace_bytes};
    RPNET_REQUIRE(rho >= 1 && rho <= RPNET_MORPH_MAX_RHO, RPNET_ERR_ARG, "%s: rho %lld (a squared radius in voxels, 1..%d)", fn, (long long)rho,
                  RPNET_MORPH_MAX_RHO);
    if (const int rc = morph_check(fn, a)) return rc;
    const MorphVox m{(int32_t)rho};
    return morph_run(fn, a, m, m, m, (hipStream_t)stream);
}

extern "C" int rpnet_morph_apply_spacing(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int op, const double* w, double r2,
                                         int per_slice, int erode_border, const void* truth, int truth_kind, int64_t* counts, int64_t counts_row,
                                         int64_t* stats, int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes,
                                         rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "morph_apply_spacing";
    const MorphArgs a{in,     kind_in,    out,   cls,       D,      H,         W,         op, per_slice != 0, erode_border != 0, truth, truth_kind,
                      counts, counts_row, stats, stats_row, n_rows, workspace, workspace_bytes};
    RPNET_REQUIRE(w, RPNET_ERR_ARG, "%s: null pointer", fn);
    for (int ax = 0; ax < 3; ++ax)
        RPNET_REQUIRE(std::isfinite(w[ax]) && w[ax] > 0.0, RPNET_ERR_ARG, "%s: weight %d is %g (every weight finite and > 0)", fn, ax, w[ax]);
    RPNET_REQUIRE(std::isfinite(r2) && r2 > 0.0, RPNET_ERR_ARG, "%s: r2 is %g (a squared radius, finite and > 0)", fn, r2);
    if (const int rc = morph_check(fn, a)) return rc;
    const double capv = std::nextafter(r2, HUGE_VAL);               // finite or +inf: either is above every value that is asked about
    return morph_run(fn, a, MorphMm{w[2], r2, capv}, MorphMm{w[1], r2, capv}, MorphMm{w[0], r2, capv}, (hipStream_t)stream);      // x, y, z
}
