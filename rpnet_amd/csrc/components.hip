// Connected components of one class of a segmented volume, and the filter that keeps the largest of them, on the device
// (include/rpnet_cc_abi.h; rpnet_amd/components.py).  Integer work only: union-find with the smallest linear index of a component as
// its root, so the labels (1 + that index) do not depend on the order in which blocks or atomics run.
//
// Launches of a call: memset (head), memset (size), local labelling, seam merge, flatten + sizes (these three in cc_phases.h, shared
// with cc_post.hip; instantiated here with the class itself as the predicate and links across z), choose, statistics row and, for
// rpnet_cc_keep_largest, filter + tally.  A tile is 4 x 32 x 64 voxels (z, y, x): a wave owns whole x runs of 64 voxels (coalesced
// 64 to 512 bytes per row, by element kind) and the tile's int32 labels are 32 KiB of LDS, five blocks per CU beside each other.
//
// Bounds.  parent[i] <= i holds from the first store on and every later store lowers parent[i] to a voxel of i's own component, so a
// find walks strictly downward and every retry of a union strictly lowers the larger of its two roots.  Every loop below therefore
// has a bound known at entry (the voxel count of the tile or of the volume) and carries it in its condition; a loop that exhausts it
// sets the head's `overrun` word and leaves.  No thread waits on another block; blocks share nothing but integer atomics.
#include "cc_phases.h"

namespace rpnet {

// Phase 5.  A root is a voxel with parent[i] == i.  The key orders by size first and by the smaller root among equal sizes.
__global__ __launch_bounds__(256) void cc_choose_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ size, const size_t n,
                                                        const int iters, CcHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned long long sbest;
    __shared__ unsigned scomp;
    const int t = threadIdx.x;
    if (t == 0) {
        sbest = 0ull;
        scomp = 0u;
    }
    __syncthreads();
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)blockIdx.x * iters + it) * 256u + t;
        if (i >= n || parent[i] != (int)i) continue;
        atomicMax(&sbest, ((unsigned long long)(unsigned)size[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
        atomicAdd(&scomp, 1u);
    }
    __syncthreads();
    if (t == 0 && scomp) {
        atomicMax(&head->best, sbest);
        atomicAdd(&head->n_comp, (unsigned long long)scomp);
    }
}

__global__ __launch_bounds__(64) void cc_stats_kernel(const CcHead* __restrict__ head, long long* __restrict__ row) {
    const int t = threadIdx.x;
    if (t >= RPNET_CC_STATS_ROW) return;
    const unsigned long long best = head->best;
    long long v;
    if (t == 0) v = (long long)head->n_fg;
    else if (t == 1) v = head->overrun ? -1ll : (long long)head->n_comp;
    else if (t == 2) v = (long long)(best >> 32);
    else v = best ? (long long)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -1ll;
    row[t] = v;
}

// Phase 6.  in and out may be one uint8 volume: a thread reads in[i] before it writes out[i] and touches no other element.
__global__ __launch_bounds__(256) void cc_filter_kernel(const void* in, const int kind, uint8_t* out, const int cls,
                                                        const int32_t* __restrict__ parent, const void* __restrict__ truth, const int truth_kind,
                                                        unsigned long long* __restrict__ counts, const size_t n, const int iters,
                                                        const CcHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned sc[3];
    const int t = threadIdx.x;
    if (t < 3) sc[t] = 0u;
    __syncthreads();
    const unsigned long long best = head->best;
    const int chosen = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -2;
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)blockIdx.x * iters + it) * 256u + t;
        if (i >= n) continue;
        const bool keep = parent[i] == chosen;
        const uint8_t v = vol_u8(in, kind, i);
        out[i] = keep ? (uint8_t)cls : (vol_fg(in, kind, i, cls) ? (uint8_t)0 : v);
        if (truth) {
            const bool tr = vol_fg(truth, truth_kind, i, cls);
            if (keep && tr) atomicAdd(&sc[0], 1u);
            if (keep) atomicAdd(&sc[1], 1u);
            if (tr) atomicAdd(&sc[2], 1u);
        }
    }
    if (!truth) return;
    __syncthreads();
    if (t < 3 && sc[t]) atomicAdd(counts + t, (unsigned long long)sc[t]);
}

// phases 1 to 5 and the statistics row; every argument has been checked
static int cc_run(const char* what, const void* vol, int kind, int cls, int D, int H, int W, int connectivity, int32_t* labels, int64_t* stats,
                  int64_t stats_row, void* workspace, hipStream_t st) {
    const size_t n = (size_t)D * H * W, vb = cc_vol_bytes(D, H, W);
    CcHead* head = static_cast<CcHead*>(workspace);
    int32_t* parent = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + kCcHeadBytes);
    int32_t* size = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + kCcHeadBytes + vb);
    if (hipMemsetAsync(head, 0, kCcHeadBytes, st) != hipSuccess || hipMemsetAsync(size, 0, vb, st) != hipSuccess) {
        const int rc = check_launch(what);
        return rc ? rc : RPNET_ERR_ARG;
    }
    const int conn26 = connectivity == 26;
    hipLaunchKernelGGL((cc_local_kernel<false, false>), dim3(cdiv(W, kCcTX), cdiv(H, kCcTY), cdiv(D, kCcTZ)), dim3(256), 0, st, vol, kind, cls, D, H, W, conn26,
                       parent, head);
    const int blocks = (int)std::min<size_t>((n + 255) / 256, (size_t)kCcBlocks);
    const int iters = (int)((n + (size_t)blocks * 256 - 1) / ((size_t)blocks * 256));
    hipLaunchKernelGGL(cc_merge_kernel<false>, dim3(blocks), dim3(256), 0, st, parent, D, H, W, conn26, FastDiv((unsigned)W), FastDiv((unsigned)H), n,
                       iters, head);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks), dim3(256), 0, st, parent, size, labels, n, iters, head);
    hipLaunchKernelGGL(cc_choose_kernel, dim3(blocks), dim3(256), 0, st, parent, size, n, iters, head);
    hipLaunchKernelGGL(cc_stats_kernel, dim3(1), dim3(64), 0, st, head, reinterpret_cast<long long*>(stats) + stats_row * RPNET_CC_STATS_ROW);
    return 0;
}

}  // namespace rpnet

extern "C" int rpnet_cc_abi_version(void) { return RPNET_CC_ABI_VERSION; }

extern "C" size_t rpnet_cc_workspace_bytes(int D, int H, int W) {
    using namespace rpnet;
    if (!cc_dims_ok(D, H, W)) {
        set_error("components: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_CC_MAX_DIM);
        return 0;
    }
    return kCcHeadBytes + 2 * cc_vol_bytes(D, H, W);
}

extern "C" int rpnet_cc_label(const void* vol, int kind, int cls, int D, int H, int W, int connectivity, int32_t* labels, int64_t* stats,
                              int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(vol && labels && stats && workspace, RPNET_ERR_ARG, "cc_label: null pointer");
    RPNET_REQUIRE(cc_kind_ok(kind), RPNET_ERR_ARG, "cc_label: element kind %d (0 uint8, 1 int32, 2 int64, 3 float32)", kind);
    RPNET_REQUIRE(connectivity == 6 || connectivity == 26, RPNET_ERR_ARG, "cc_label: connectivity %d (6 or 26)", connectivity);
    RPNET_REQUIRE(cc_dims_ok(D, H, W), RPNET_ERR_SHAPE, "cc_label: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(n_rows >= 1 && stats_row >= 0 && stats_row < n_rows, RPNET_ERR_ARG, "cc_label: row %lld of a table of %lld rows",
                  (long long)stats_row, (long long)n_rows);
    const size_t need = rpnet_cc_workspace_bytes(D, H, W);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "cc_label: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)vol % kCcElem[kind]) == 0 && ((uintptr_t)labels % 4) == 0 && ((uintptr_t)stats % 8) == 0 &&
                      ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "cc_label: the volume must be aligned to its element, the labels to 4, the table to 8 and the workspace to 16 bytes");
    const int rc = cc_run("cc_label (memset)", vol, kind, cls, D, H, W, connectivity, labels, stats, stats_row, workspace, (hipStream_t)stream);
    return rc ? rc : check_launch("cc_label");
}

extern "C" int rpnet_cc_keep_largest(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int connectivity, const void* truth,
                                     int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats, int64_t stats_row, int64_t n_rows,
                                     void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(in && out && stats && workspace, RPNET_ERR_ARG, "cc_keep_largest: null pointer");
    RPNET_REQUIRE((truth == nullptr) == (counts == nullptr), RPNET_ERR_ARG, "cc_keep_largest: truth and counts come together (both or neither)");
    RPNET_REQUIRE(cc_kind_ok(kind_in) && (!truth || cc_kind_ok(truth_kind)), RPNET_ERR_ARG,
                  "cc_keep_largest: element kinds %d, %d (0 uint8, 1 int32, 2 int64, 3 float32)", kind_in, truth_kind);
    RPNET_REQUIRE(connectivity == 6 || connectivity == 26, RPNET_ERR_ARG, "cc_keep_largest: connectivity %d (6 or 26)", connectivity);
    RPNET_REQUIRE(cls >= 1 && cls <= 255, RPNET_ERR_ARG, "cc_keep_largest: class %d (1..255: the output is uint8)", cls);
    RPNET_REQUIRE(cc_dims_ok(D, H, W), RPNET_ERR_SHAPE, "cc_keep_largest: D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(n_rows >= 1 && stats_row >= 0 && stats_row < n_rows && (!counts || (counts_row >= 0 && counts_row < n_rows)), RPNET_ERR_ARG,
                  "cc_keep_largest: rows %lld and %lld of tables of %lld rows", (long long)counts_row, (long long)stats_row, (long long)n_rows);
    const size_t need = rpnet_cc_workspace_bytes(D, H, W);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "cc_keep_largest: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)in % kCcElem[kind_in]) == 0 && (!truth || ((uintptr_t)truth % kCcElem[truth_kind]) == 0) &&
                      ((uintptr_t)stats % 8) == 0 && ((uintptr_t)counts % 8) == 0 && ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "cc_keep_largest: volumes must be aligned to their element, the tables to 8 and the workspace to 16 bytes");
    const size_t n = (size_t)D * H * W;
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + n * kCcElem[kind_in], b0 = (uintptr_t)out, b1 = b0 + n;
    RPNET_REQUIRE((kind_in == RPNET_CC_U8 && a0 == b0) || a1 <= b0 || b1 <= a0, RPNET_ERR_ARG,
                  "cc_keep_largest: out overlaps in (only a uint8 volume can be filtered in place, out == in)");

    const hipStream_t st = (hipStream_t)stream;
    const int rc = cc_run("cc_keep_largest (memset)", in, kind_in, cls, D, H, W, connectivity, nullptr, stats, stats_row, workspace, st);
    if (rc) return rc;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, (size_t)kCcBlocks);
    const int iters = (int)((n + (size_t)blocks * 256 - 1) / ((size_t)blocks * 256));
    const int32_t* parent = reinterpret_cast<const int32_t*>(static_cast<char*>(workspace) + kCcHeadBytes);
    hipLaunchKernelGGL(cc_filter_kernel, dim3(blocks), dim3(256), 0, st, in, kind_in, out, cls, parent, truth, truth_kind,
                       counts ? reinterpret_cast<unsigned long long*>(counts) + counts_row * RPNET_CC_COUNTS_ROW : nullptr, n, iters,
                       static_cast<const CcHead*>(workspace));
    return check_launch("cc_keep_largest");
}
