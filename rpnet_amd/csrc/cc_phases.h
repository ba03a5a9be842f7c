// The phases the connected-component entry points (components.hip, include/rpnet_cc_abi.h) and the post-processing entry points
// (cc_post.hip, include/rpnet_ccpost_abi.h) share: the tile constants, the head of a workspace, union-find in LDS
// and in global memory, local labelling, the seam merge and flatten + sizes.  The local labelling and the seam merge are templates:
//   kComplement  the labelled voxels are those with `value != cls` (the background of a class) instead of `value == cls`;
//   kPlanar      no link has a z component: every z slice is its own 2D image (no z joins inside the tile, no z seams), so
//                connectivity 6 / 26 acts as its in-plane subset 4 / 8.
// components.hip instantiates <false, false>: both switches are compile-time constants that fold away, the code it had before the split.
#ifndef RPNET_CC_PHASES_H
#define RPNET_CC_PHASES_H

#include <algorithm>

#include "rpnet_cc_abi.h"
#include "volume_kinds.h"

namespace rpnet {

constexpr int kCcLX = 6, kCcLY = 5, kCcLZ = 2;                  // log2 of the tile extents
constexpr int kCcTX = 1 << kCcLX, kCcTY = 1 << kCcLY, kCcTZ = 1 << kCcLZ;
constexpr int kCcTile = kCcTX * kCcTY * kCcTZ;                  // 8192 voxels, 32 KiB of int32
constexpr int kCcBlocks = 8192;                                 // blocks of a per-voxel sweep at most
constexpr int kCcSlots = 128;                                   // (root, count) pairs a block gathers in LDS before it adds to size[]
constexpr size_t kCcHeadBytes = 64;
static_assert(kCcTX == 64, "a wave's ballot labels one x run of the tile");
static_assert(kCcTile * sizeof(int) <= 32 * 1024, "LDS of a tile");
static_assert((long long)RPNET_CC_MAX_DIM * RPNET_CC_MAX_DIM * RPNET_CC_MAX_DIM < (1ll << 31), "a linear index must fit int32");

struct CcHead {                         // the first 64 bytes of a workspace, cleared before the first launch that reads it (components.hip: a memset; cc_post.hip: a launch)
    unsigned long long best;            // max over the roots of (size << 32) | (0xFFFFFFFF - root)
    unsigned long long n_fg, n_comp;
    unsigned overrun;                   // RPNET_CC_OVERRUN_OFFSET
    unsigned pad;
    unsigned long long post[4];         // cc_post.hip: n_selected, voxels, largest_selected, spare
};
static_assert(sizeof(CcHead) == kCcHeadBytes && offsetof(CcHead, overrun) == RPNET_CC_OVERRUN_OFFSET, "head layout");

static_assert(RPNET_CC_U8 == RPNET_SURFACE_U8 && RPNET_CC_I32 == RPNET_SURFACE_I32 && RPNET_CC_I64 == RPNET_SURFACE_I64 &&
                  RPNET_CC_F32 == RPNET_SURFACE_F32,
              "vol_fg and vol_u8 of volume_kinds.h switch over the element kinds of both headers");

// is (dz, dy, dx) one of the lower half of the neighbourhood (the neighbours that come before a voxel in z-major order)?
__host__ __device__ constexpr bool cc_lower(const int dz, const int dy, const int dx) {
    return dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
}
__host__ __device__ constexpr bool cc_face(const int dz, const int dy, const int dx) { return dz * dz + dy * dy + dx * dx == 1; }

// ------------------------------------------------------------------------------------------------------ union-find in LDS
__device__ __forceinline__ int cc_lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// root of a (lab[a] >= 0): at most kCcTile steps, each strictly downward; the start is then pointed at the root (atomicMin: never up)
__device__ __forceinline__ int cc_find_lds(int* lab, const int start, unsigned* overrun) {
    int a = start;
    bool done = false;
    for (int it = 0; it < kCcTile; ++it) {
        const int p = cc_lds_load(lab + a);
        if (p == a) {
            done = true;
            break;
        }
        a = p;
    }
    if (!done) atomicOr(overrun, 1u);
    if (a != start) atomicMin(lab + start, a);
    return a;
}

// at most kCcTile retries: a retry continues from `old` < a, so the larger of the two roots falls every time
__device__ __forceinline__ void cc_union_lds(int* lab, int a, int b, unsigned* overrun) {
    for (int it = 0; it < kCcTile; ++it) {
        a = cc_find_lds(lab, a, overrun);
        b = cc_find_lds(lab, b, overrun);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;               // a was a root and now points at b
        a = old;                            // a had been linked to old < a meanwhile: unite old and b
    }
    atomicOr(overrun, 1u);
}

// Phase 1.  grid (ceil(W / 64), ceil(H / 32), ceil(D / 4)).  Local index l = (zl * 32 + yl) * 64 + xl grows with the global linear
// index, so the smallest local index of a component of the tile is its smallest global one.
template <bool kComplement, bool kPlanar>
__global__ __launch_bounds__(256) void cc_local_kernel(const void* __restrict__ vol, const int kind, const int cls, const int D, const int H,
                                                       const int W, const int conn26, int32_t* __restrict__ parent, CcHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ int lab[kCcTile];
    const int t = threadIdx.x, lane = t & (kCcTX - 1);
    const int x0 = blockIdx.x << kCcLX, y0 = blockIdx.y << kCcLY, z0 = blockIdx.z << kCcLZ;
    const int x = x0 + lane;

    // the x runs, from the wave's ballot: l & 63 == lane, so a wave holds one row of the tile per step
    for (int k = 0; k < kCcTile / 256; ++k) {
        const int l = t + 256 * k;
        const int y = y0 + ((l >> kCcLX) & (kCcTY - 1)), z = z0 + (l >> (kCcLX + kCcLY));
        const bool f = x < W && y < H && z < D && vol_fg(vol, kind, ((size_t)z * H + y) * W + x, cls) != kComplement;
        const unsigned long long m = __ballot(f);
        const unsigned long long gaps = ~m & ((1ull << lane) - 1ull);          // background voxels of the row before this one
        const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
        lab[l] = f ? l - lane + start : -1;
    }
    __syncthreads();

    // join the runs across y and z inside the tile (and across x diagonally, for 26)
    for (int k = 0; k < kCcTile / 256; ++k) {
        const int l = t + 256 * k;
        if (lab[l] < 0) continue;
        const int yl = (l >> kCcLX) & (kCcTY - 1), zl = l >> (kCcLX + kCcLY);
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_lower(dz, dy, dx) || (dz == 0 && dy == 0)) continue;          // (0, 0, -1) is the run itself
                    if (!conn26 && !cc_face(dz, dy, dx)) continue;
                    if (kPlanar && dz != 0) continue;
                    const int nx = lane + dx, ny = yl + dy, nz = zl + dz;
                    if (nx < 0 || nx >= kCcTX || ny < 0 || ny >= kCcTY || nz < 0) continue;
                    const int nl = l + (dz << (kCcLX + kCcLY)) + (dy << kCcLX) + dx;
                    if (cc_lds_load(lab + nl) < 0) continue;
                    cc_union_lds(lab, l, nl, &head->overrun);
                }
    }
    __syncthreads();

    for (int k = 0; k < kCcTile / 256; ++k) {
        const int l = t + 256 * k;
        const int y = y0 + ((l >> kCcLX) & (kCcTY - 1)), z = z0 + (l >> (kCcLX + kCcLY));
        if (x >= W || y >= H || z >= D) continue;
        int g = -1;
        if (lab[l] >= 0) {
            const int r = cc_find_lds(lab, l, &head->overrun);
            g = ((z0 + (r >> (kCcLX + kCcLY))) * H + y0 + ((r >> kCcLX) & (kCcTY - 1))) * W + x0 + (r & (kCcTX - 1));
        }
        parent[((size_t)z * H + y) * W + x] = g;
    }
}

// ------------------------------------------------------------------------------------------- union-find in global memory
// Inside the merge launch other blocks, on other XCDs, lower entries of parent[] while this one reads them, and the XCDs' L2s are
// not coherent for plain loads: every read is a device-scope atomic load and every write the atomicMin, which acts on what memory
// holds.  Every value parent[a] ever holds is a voxel of a's component with an index <= a, and it only falls.  A stale read is
// therefore an earlier, larger member of the same component: a find that follows it ends at a voxel of the right component, which
// may no longer be a root; the atomicMin on it then returns something else than it, and the union retries from there (one more
// iteration).  Linking two voxels of one true component is never a wrong merge, and the link is only taken as made (`old == a`) on
// the atomic's own return value.
__device__ __forceinline__ int cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(const int32_t* parent, int a, const unsigned bound, unsigned* overrun) {
    for (unsigned it = 0; it < bound; ++it) {
        const int p = cc_load(parent + a);
        if (p == a) return a;
        a = p;
    }
    atomicOr(overrun, 1u);
    return a;
}

__device__ __forceinline__ void cc_union(int32_t* parent, int a, int b, const unsigned bound, unsigned* overrun) {
    for (unsigned it = 0; it < bound; ++it) {
        a = cc_find(parent, a, bound, overrun);
        b = cc_find(parent, b, bound, overrun);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(overrun, 1u);
}

// Phase 2.  One thread per voxel, `iters` sweeps of 256 consecutive voxels per block.  Only a voxel on a face of its tile can have a
// lower neighbour in another tile (the low faces; for 26 the high x and y faces too: (dy, dx) = (-1, +1) and (dz, dy) = (-1, +1)).
// kPlanar: no neighbour with dz != 0, so the low z face of a tile is no seam.
template <bool kPlanar>
__global__ __launch_bounds__(256) void cc_merge_kernel(int32_t* parent, const int D, const int H, const int W, const int conn26,
                                                       const FastDiv div_w, const FastDiv div_h, const size_t n, const int iters,
                                                       CcHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    const int HW = H * W;
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)blockIdx.x * iters + it) * 256u + threadIdx.x;
        if (i >= n) continue;
        unsigned q, zz;
        const int x = (int)div_w.divmod((unsigned)i, q);
        const int y = (int)div_h.divmod(q, zz);
        const int z = (int)zz;
        const int xl = x & (kCcTX - 1), yl = y & (kCcTY - 1), zl = z & (kCcTZ - 1);
        const bool edge = xl == 0 || yl == 0 || (!kPlanar && zl == 0) || (conn26 && (xl == kCcTX - 1 || yl == kCcTY - 1));
        if (!edge || cc_load(parent + i) < 0) continue;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_lower(dz, dy, dx)) continue;
                    if (!conn26 && !cc_face(dz, dy, dx)) continue;
                    if (kPlanar && dz != 0) continue;
                    const int nx = x + dx, ny = y + dy, nz = z + dz;
                    if (nx < 0 || nx >= W || ny < 0 || ny >= H || nz < 0) continue;
                    if ((nx >> kCcLX) == (x >> kCcLX) && (ny >> kCcLY) == (y >> kCcLY) && (nz >> kCcLZ) == (z >> kCcLZ)) continue;
                    const int j = (int)i + dz * HW + dy * W + dx;
                    if (cc_load(parent + j) < 0) continue;
                    cc_union(parent, (int)i, j, (unsigned)n, &head->overrun);
                }
    }
}

// Phases 3 and 4.  parent[i] = root of i, in place, by plain accesses: another block may store the root of j while this one walks
// through parent[j]; it reads the earlier value or the root, both voxels of the component with an index <= j (see above), so the
// walk still ends at the root — the merge launch is complete, and no root changes here.  size[root] += 1: a block gathers the
// counts of the roots it meets in a small LDS table (a slot belongs to the first root that claims it; a root that finds its slot
// taken adds to size[] directly), then adds every slot once.
static __global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* parent, int32_t* __restrict__ size, int32_t* __restrict__ labels,
                                                         const size_t n, const int iters, CcHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ int skey[kCcSlots];
    __shared__ unsigned scnt[kCcSlots];
    __shared__ unsigned sfg;
    const int t = threadIdx.x;
    if (t < kCcSlots) {
        skey[t] = -1;
        scnt[t] = 0u;
    }
    if (t == 0) sfg = 0u;
    __syncthreads();
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)blockIdx.x * iters + it) * 256u + t;
        if (i >= n) continue;
        const int p = parent[i];
        int r = -1;
        if (p >= 0) {
            r = p;
            bool done = false;
            for (unsigned s = 0; s < (unsigned)n; ++s) {
                const int pp = parent[r];
                if (pp == r) {
                    done = true;
                    break;
                }
                r = pp;
            }
            if (!done) atomicOr(&head->overrun, 1u);
            if (r != p) parent[i] = r;
            atomicAdd(&sfg, 1u);
            const int slot = (r ^ (r >> 7) ^ (r >> 14) ^ (r >> 21)) & (kCcSlots - 1);
            const int prev = atomicCAS(&skey[slot], -1, r);
            if (prev == -1 || prev == r) atomicAdd(&scnt[slot], 1u);
            else atomicAdd(size + r, 1);
        }
        if (labels) labels[i] = r + 1;
    }
    __syncthreads();
    if (t < kCcSlots && skey[t] >= 0) atomicAdd(size + skey[t], (int)scnt[t]);
    if (t == 0 && sfg) atomicAdd(&head->n_fg, (unsigned long long)sfg);
}

static inline size_t cc_vol_bytes(int D, int H, int W) { return ((size_t)D * H * W * sizeof(int32_t) + 15) / 16 * 16; }
static inline bool cc_dims_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= RPNET_CC_MAX_DIM && H <= RPNET_CC_MAX_DIM && W <= RPNET_CC_MAX_DIM;
}
static inline bool cc_kind_ok(int kind) { return kind >= RPNET_CC_U8 && kind <= RPNET_CC_F32; }
static const size_t kCcElem[4] = {1, 4, 8, 4};

// blocks and sweeps per block of a per-voxel launch over n voxels
static inline int cc_sweep_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, (size_t)kCcBlocks); }
static inline int cc_sweep_iters(size_t n, int blocks) { return (int)((n + (size_t)blocks * 256 - 1) / ((size_t)blocks * 256)); }

}  // namespace rpnet
#endif  // RPNET_CC_PHASES_H
