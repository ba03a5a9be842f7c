// Post-processing of one class of a segmented volume on the device: fill its holes, remove its small components
// (include/rpnet_ccpost_abi.h; rpnet_amd/postprocess.py).  Both are predicates over component labels, so the labelling is that of
// components.hip, shared through cc_phases.h: local labelling in LDS, the seam merge, flatten + sizes.  A hole is a component of the
// complement (`value != cls`) that does not reach the border; a small component is one of `value == cls` below a size.
//
// Launches of rpnet_ccpost_fill_holes: clear (head and size), local labelling <complement, planar?>, seam merge <planar?>,
// flatten + sizes, border, fill + tally, statistics row.  rpnet_ccpost_remove_small: the same without the border launch, on the class
// itself.  Integer work only; nothing depends on the order of blocks or atomics.
//
// The border mark is the sign bit of size[root]: a component has at most 2^30 voxels (RPNET_CC_MAX_DIM^3), so the atomicAdds of the
// flatten launch never carry into bit 31, and the border launch sets it by an atomicOr of one constant, which is idempotent.  The fill
// launch then reads one word per root: negative = reaches the border, otherwise the size.
//
// Bounds.  The loops of cc_phases.h carry theirs (the voxel count of the tile or of the volume).  The launches of this file hold no
// walk at all: after the flatten launch parent[i] is the root of i, so the border and the apply launches read parent once per voxel;
// their only loops are the sweeps of a block (`iters`) and the 16 voxels of a lane.
#include <climits>

#include "cc_phases.h"
#include "rpnet_ccpost_abi.h"

namespace rpnet {

constexpr unsigned kPostBorderBit = 0x80000000u;
constexpr int kPostLane = 16;                       // voxels of a lane in the apply launch: one 16-byte store of out
static_assert(RPNET_CCPOST_OVERRUN_OFFSET == RPNET_CC_OVERRUN_OFFSET, "the head is that of components.hip");
static_assert((long long)RPNET_CC_MAX_DIM * RPNET_CC_MAX_DIM * RPNET_CC_MAX_DIM <= (1ll << 30), "a size must leave bit 31 free");

// Clear.  The head and the size volume are cleared by a launch, not by hipMemsetAsync: captured in a graph, the memset node of such a
// head has come back with stale bytes on replay (surface_spacing.hip met the same), while a kernel's arguments are part of its node.
// n16: the 16-byte words of the size volume (its bytes are a multiple of 16 and it starts 16-byte aligned inside the workspace).
__global__ __launch_bounds__(256) void post_clear_kernel(uint4* __restrict__ head, uint4* __restrict__ size, const size_t n16, const int iters) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x < kCcHeadBytes / sizeof(uint4)) head[threadIdx.x] = zero;
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)blockIdx.x * iters + it) * 256u + threadIdx.x;
        if (i < n16) size[i] = zero;
    }
}

// Border.  One thread per voxel of the faces: n_z = 2*H*W voxels of z = 0 and z = D - 1 (0 in per-slice mode), then n_y = 2*D*W of
// y = 0 and y = H - 1, then 2*D*H of x = 0 and x = W - 1; a voxel on an edge is visited more than once, which the mark does not notice.
// Every index is (z*H + y)*W + x with z < D, y < H, x < W.  The read before the atomicOr only spares the atomics of a root that
// is marked already (the outside, as a rule); it is a device-scope load, and a stale value costs one more atomicOr of the same bit.
// Neighbouring face voxels mostly share a root (the outside), and a load and an atomic per voxel on that one word serialise: of a run
// of lanes with the same root only the first speaks (every distinct root of a wave still has a lane that does), which took
// 1.4 ms off the 3D call on a 64 x 256 x 256 final mask (profiles/postprocess_eval.txt).
__global__ __launch_bounds__(256) void post_border_kernel(const int32_t* __restrict__ parent, int32_t* size, const int D, const int H, const int W,
                                                          const unsigned n_z, const unsigned n_y, const unsigned total) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    unsigned x = 0u, y = 0u, z = 0u;
    if (t >= total) {
    } else if (t < n_z) {
        const unsigned plane = (unsigned)H * (unsigned)W, side = t / plane, r = t - side * plane;
        z = side ? (unsigned)D - 1u : 0u;
        y = r / (unsigned)W;
        x = r - y * (unsigned)W;
    } else if (t < n_z + n_y) {
        const unsigned u = t - n_z, row = 2u * (unsigned)W, r = u % row;
        z = u / row;
        y = r >= (unsigned)W ? (unsigned)H - 1u : 0u;
        x = r >= (unsigned)W ? r - (unsigned)W : r;
    } else {
        const unsigned u = t - n_z - n_y, row = 2u * (unsigned)H, r = u % row;
        z = u / row;
        x = r >= (unsigned)H ? (unsigned)W - 1u : 0u;
        y = r >= (unsigned)H ? r - (unsigned)H : r;
    }
    const int p = t < total ? parent[((size_t)z * H + y) * W + x] : -1;
    const int before = __shfl_up(p, 1);                        // every lane of the wave is here: no lane has returned
    const bool speaks = (threadIdx.x & 63u) == 0u || before != p;
    if (p >= 0 && speaks && cc_load(size + p) >= 0) atomicOr(reinterpret_cast<unsigned*>(size) + p, kPostBorderBit);
}

// Fill (kHoles) or remove (!kHoles) and tally.  A lane owns kPostLane consecutive voxels: it reads them, then writes them (one
// 16-byte store where `vec` says that out is 16-byte aligned and the lane's voxels are all inside the volume), and touches no other
// element of in or out, so the two may be one uint8 volume.  `lim`: kHoles: a component of the complement with a clear border bit and
// a size <= lim is a hole (INT_MAX: no bound); !kHoles: a component of the class with a size < lim is removed.
// Head: n_comp the components, post[0] the selected ones (holes / removed), post[1] the voxels written, post[2] the largest selected size.
template <bool kHoles>
__global__ __launch_bounds__(256) void post_apply_kernel(const void* in, const int kind, uint8_t* out, const int cls, const int32_t* __restrict__ parent,
                                                         const int32_t* __restrict__ size, const int lim, const void* truth, const int truth_kind,
                                                         unsigned long long* __restrict__ counts, const size_t n, const size_t n_lanes,
                                                         const int iters, const int vec, CcHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned sc[7];                      // n_comp, n_selected, voxels, largest, |P and T|, |P|, |T|
    const int t = threadIdx.x;
    if (t < 7) sc[t] = 0u;
    __syncthreads();
    unsigned ncomp = 0u, nsel = 0u, vox = 0u, largest = 0u, c_pt = 0u, c_p = 0u, c_t = 0u;
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)blockIdx.x * iters + it) * 256u + t;
        if (lane >= n_lanes) continue;
        const size_t base = lane * kPostLane;
        const int cnt = (int)std::min<size_t>((size_t)kPostLane, n - base);
        union {
            uint8_t b[kPostLane];
            uint4 q;
        } o;
        int last_p = -1, last_s = 0;
#pragma unroll
        for (int j = 0; j < kPostLane; ++j) {
            if (j >= cnt) continue;
            const size_t i = base + j;
            const int p = parent[i];
            const uint8_t v = vol_u8(in, kind, i);
            bool sel = false;
            if (p >= 0) {
                if (p != last_p) {
                    last_p = p;
                    last_s = size[p];
                }
                const int s = last_s;
                sel = kHoles ? (s >= 0 && s <= lim) : s < lim;
                if (p == (int)i) {                  // the root speaks for its component
                    ++ncomp;
                    if (sel) {
                        ++nsel;
                        largest = max(largest, (unsigned)s);
                        if (!kHoles) vox += (unsigned)s;
                    }
                }
            }
            bool pred;                              // does the result hold the class here?
            if (kHoles) {
                const bool fill = sel && vol_fg(in, kind, i, 0);          // only a voxel of value 0 is filled
                if (fill) ++vox;
                o.b[j] = fill ? (uint8_t)cls : v;
                pred = p < 0 || fill;
            } else {
                o.b[j] = p >= 0 ? (sel ? (uint8_t)0 : (uint8_t)cls) : v;
                pred = p >= 0 && !sel;
            }
            if (truth) {
                const bool tr = vol_fg(truth, truth_kind, i, cls);
                c_pt += pred && tr;
                c_p += pred;
                c_t += tr;
            }
        }
        if (vec && cnt == kPostLane) {
            *reinterpret_cast<uint4*>(out + base) = o.q;
        } else {
            for (int j = 0; j < cnt; ++j) out[base + j] = o.b[j];
        }
    }
    if (ncomp) atomicAdd(&sc[0], ncomp);
    if (nsel) atomicAdd(&sc[1], nsel);
    if (vox) atomicAdd(&sc[2], vox);
    if (largest) atomicMax(&sc[3], largest);
    if (c_pt) atomicAdd(&sc[4], c_pt);
    if (c_p) atomicAdd(&sc[5], c_p);
    if (c_t) atomicAdd(&sc[6], c_t);
    __syncthreads();
    if (t == 0 && sc[0]) atomicAdd(&head->n_comp, (unsigned long long)sc[0]);
    if ((t == 1 || t == 2) && sc[t]) atomicAdd(&head->post[t - 1], (unsigned long long)sc[t]);
    if (t == 3 && sc[3]) atomicMax(&head->post[2], (unsigned long long)sc[3]);
    if (t >= 4 && t < 7 && counts && sc[t]) atomicAdd(counts + (t - 4), (unsigned long long)sc[t]);
}

__global__ __launch_bounds__(64) void post_stats_kernel(const CcHead* __restrict__ head, long long* __restrict__ row) {
    const int t = threadIdx.x;
    if (t >= RPNET_CCPOST_STATS_ROW) return;
    row[t] = t == 0 ? (head->overrun ? -1ll : (long long)head->n_comp) : (long long)head->post[t - 1];
}

struct PostArgs {
    const void* in;
    int kind_in;
    uint8_t* out;
    int cls, D, H, W;
    const void* truth;
    int truth_kind;
    int64_t *counts, counts_row, *stats, stats_row, n_rows;
    void* workspace;
    size_t workspace_bytes;
};

// the refusals the two entry points share; `fn` names the entry point in the message
static int post_check(const char* fn, const PostArgs& a) {
    RPNET_REQUIRE(a.in && a.out && a.stats && a.workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE((a.truth == nullptr) == (a.counts == nullptr), RPNET_ERR_ARG, "%s: truth and counts come together (both or neither)", fn);
    RPNET_REQUIRE(cc_kind_ok(a.kind_in) && (!a.truth || cc_kind_ok(a.truth_kind)), RPNET_ERR_ARG,
                  "%s: element kinds %d, %d (0 uint8, 1 int32, 2 int64, 3 float32)", fn, a.kind_in, a.truth_kind);
    RPNET_REQUIRE(a.cls >= 1 && a.cls <= 255, RPNET_ERR_ARG, "%s: class %d (1..255: the output is uint8)", fn, a.cls);
    RPNET_REQUIRE(cc_dims_ok(a.D, a.H, a.W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, a.D, a.H, a.W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(a.n_rows >= 1 && a.stats_row >= 0 && a.stats_row < a.n_rows && (!a.counts || (a.counts_row >= 0 && a.counts_row < a.n_rows)),
                  RPNET_ERR_ARG, "%s: rows %lld and %lld of tables of %lld rows", fn, (long long)a.counts_row, (long long)a.stats_row,
                  (long long)a.n_rows);
    const size_t need = kCcHeadBytes + 2 * cc_vol_bytes(a.D, a.H, a.W);
    RPNET_REQUIRE(a.workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, a.workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)a.in % kCcElem[a.kind_in]) == 0 && (!a.truth || ((uintptr_t)a.truth % kCcElem[a.truth_kind]) == 0) &&
                      ((uintptr_t)a.stats % 8) == 0 && ((uintptr_t)a.counts % 8) == 0 && ((uintptr_t)a.workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: volumes must be aligned to their element, the tables to 8 and the workspace to 16 bytes", fn);
    const size_t n = (size_t)a.D * a.H * a.W;
    const uintptr_t a0 = (uintptr_t)a.in, a1 = a0 + n * kCcElem[a.kind_in], b0 = (uintptr_t)a.out, b1 = b0 + n;
    RPNET_REQUIRE((a.kind_in == RPNET_CC_U8 && a0 == b0) || a1 <= b0 || b1 <= a0, RPNET_ERR_ARG,
                  "%s: out overlaps in (only a uint8 volume can be processed in place, out == in)", fn);
    return 0;
}

// every argument has been checked.  complement / planar choose the instantiation of the shared phases; border: the border launch
template <bool kHoles>
static int post_run(const char* fn, const PostArgs& a, const bool planar, const int conn26, const int lim, hipStream_t st) {
    const size_t n = (size_t)a.D * a.H * a.W, vb = cc_vol_bytes(a.D, a.H, a.W);
    CcHead* head = static_cast<CcHead*>(a.workspace);
    int32_t* parent = reinterpret_cast<int32_t*>(static_cast<char*>(a.workspace) + kCcHeadBytes);
    int32_t* size = reinterpret_cast<int32_t*>(static_cast<char*>(a.workspace) + kCcHeadBytes + vb);
    const size_t n16 = vb / sizeof(uint4);
    const int cblocks = cc_sweep_blocks(n16);
    hipLaunchKernelGGL(post_clear_kernel, dim3(cblocks), dim3(256), 0, st, reinterpret_cast<uint4*>(head), reinterpret_cast<uint4*>(size), n16,
                       cc_sweep_iters(n16, cblocks));
    const dim3 tiles(cdiv(a.W, kCcTX), cdiv(a.H, kCcTY), cdiv(a.D, kCcTZ));
    const int blocks = cc_sweep_blocks(n), iters = cc_sweep_iters(n, blocks);
    const FastDiv div_w((unsigned)a.W), div_h((unsigned)a.H);
    if (!kHoles) {
        hipLaunchKernelGGL((cc_local_kernel<false, false>), tiles, dim3(256), 0, st, a.in, a.kind_in, a.cls, a.D, a.H, a.W, conn26, parent, head);
        hipLaunchKernelGGL(cc_merge_kernel<false>, dim3(blocks), dim3(256), 0, st, parent, a.D, a.H, a.W, conn26, div_w, div_h, n, iters, head);
    } else if (planar) {
        hipLaunchKernelGGL((cc_local_kernel<true, true>), tiles, dim3(256), 0, st, a.in, a.kind_in, a.cls, a.D, a.H, a.W, conn26, parent, head);
        hipLaunchKernelGGL(cc_merge_kernel<true>, dim3(blocks), dim3(256), 0, st, parent, a.D, a.H, a.W, conn26, div_w, div_h, n, iters, head);
    } else {
        hipLaunchKernelGGL((cc_local_kernel<true, false>), tiles, dim3(256), 0, st, a.in, a.kind_in, a.cls, a.D, a.H, a.W, conn26, parent, head);
        hipLaunchKernelGGL(cc_merge_kernel<false>, dim3(blocks), dim3(256), 0, st, parent, a.D, a.H, a.W, conn26, div_w, div_h, n, iters, head);
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks), dim3(256), 0, st, parent, size, static_cast<int32_t*>(nullptr), n, iters, head);
    if (kHoles) {
        const unsigned n_z = planar ? 0u : 2u * (unsigned)a.H * (unsigned)a.W, n_y = 2u * (unsigned)a.D * (unsigned)a.W;
        const unsigned total = n_z + n_y + 2u * (unsigned)a.D * (unsigned)a.H;              // at most 6 * 2^20
        hipLaunchKernelGGL(post_border_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, parent, size, a.D, a.H, a.W, n_z, n_y, total);
    }
    const size_t n_lanes = (n + kPostLane - 1) / kPostLane;
    const int ablocks = cc_sweep_blocks(n_lanes), aiters = cc_sweep_iters(n_lanes, ablocks);
    hipLaunchKernelGGL(post_apply_kernel<kHoles>, dim3(ablocks), dim3(256), 0, st, a.in, a.kind_in, a.out, a.cls, parent, size, lim, a.truth,
                       a.truth_kind, a.counts ? reinterpret_cast<unsigned long long*>(a.counts) + a.counts_row * RPNET_CCPOST_COUNTS_ROW : nullptr, n,
                       n_lanes, aiters, (int)(((uintptr_t)a.out % 16) == 0), head);
    hipLaunchKernelGGL(post_stats_kernel, dim3(1), dim3(64), 0, st, head,
                       reinterpret_cast<long long*>(a.stats) + a.stats_row * RPNET_CCPOST_STATS_ROW);
    return check_launch(fn);
}

}  // namespace rpnet

extern "C" int rpnet_ccpost_abi_version(void) { return RPNET_CCPOST_ABI_VERSION; }

extern "C" size_t rpnet_ccpost_workspace_bytes(int D, int H, int W) {
    using namespace rpnet;
    if (!cc_dims_ok(D, H, W)) {
        set_error("ccpost: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_CC_MAX_DIM);
        return 0;
    }
    return kCcHeadBytes + 2 * cc_vol_bytes(D, H, W);
}

extern "C" int rpnet_ccpost_fill_holes(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int bg_connectivity, int per_slice,
                                       int64_t max_hole_voxels, const void* truth, int truth_kind, int64_t* counts, int64_t counts_row,
                                       int64_t* stats, int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes,
                                       rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "ccpost_fill_holes";
    const PostArgs a{in, kind_in, out, cls, D, H, W, truth, truth_kind, counts, counts_row, stats, stats_row, n_rows, workspace, workspace_bytes};
    if (per_slice)
        RPNET_REQUIRE(bg_connectivity == 4 || bg_connectivity == 8, RPNET_ERR_ARG, "%s: background connectivity %d (4 or 8 per slice)", fn,
                      bg_connectivity);
    else
        RPNET_REQUIRE(bg_connectivity == 6 || bg_connectivity == 26, RPNET_ERR_ARG, "%s: background connectivity %d (6 or 26)", fn, bg_connectivity);
    RPNET_REQUIRE(max_hole_voxels >= 0, RPNET_ERR_ARG, "%s: max_hole_voxels %lld (0: no bound, or a positive size)", fn, (long long)max_hole_voxels);
    const int rc = post_check(fn, a);
    if (rc) return rc;
    const int lim = max_hole_voxels == 0 || max_hole_voxels > (int64_t)INT_MAX ? INT_MAX : (int)max_hole_voxels;
    return post_run<true>(fn, a, per_slice != 0, bg_connectivity == 26 || bg_connectivity == 8, lim, (hipStream_t)stream);
}

extern "C" int rpnet_ccpost_remove_small(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int connectivity, int64_t min_voxels,
                                         const void* truth, int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats, int64_t stats_row,
                                         int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "ccpost_remove_small";
    const PostArgs a{in, kind_in, out, cls, D, H, W, truth, truth_kind, counts, counts_row, stats, stats_row, n_rows, workspace, workspace_bytes};
    RPNET_REQUIRE(connectivity == 6 || connectivity == 26, RPNET_ERR_ARG, "%s: connectivity %d (6 or 26)", fn, connectivity);
    RPNET_REQUIRE(min_voxels >= 1, RPNET_ERR_ARG, "%s: min_voxels %lld (at least 1)", fn, (long long)min_voxels);
    const int rc = post_check(fn, a);
    if (rc) return rc;
    const int lim = min_voxels > (int64_t)INT_MAX ? INT_MAX : (int)min_voxels;
    return post_run<false>(fn, a, false, connectivity == 26, lim, (hipStream_t)stream);
}
