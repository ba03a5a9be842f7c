// The reader's deterministic preprocessing of a volume on the device (include/rpnet_volload_abi.h; rpnet_amd/volume_load.py): the annotated
// z range of a mask, the gather that composes truncate, pad to 16, z range, centre crop and symmetric pad, two exact order statistics of a
// float32 array, and the percentile clip, HU clip and map to [-1, 1].
//
// What was chosen.
//  - range: three launches.  The scan reads the mask as flat memory, 16 bytes per lane; only a non-zero element pays for the divisions
//    that turn its memory index into (z, y, x).  A block gathers first / last / count in LDS with integer atomics and adds them to the row
//    once.
//  - gather: one launch, a lane per 4 consecutive x of the output, one 16-byte store.  For a z-fastest source (the payload of a file) the
//    four reads of a lane stand D * H elements apart: the reads are not coalesced along x, and no LDS transpose tile is built here; the
//    neighbours along z that share a line are served by the caches.  tools/bench_volume_load.py measures it as it is.
//  - select: a most-significant-digit radix selection over the order-preserving key, 8 bits a pass, both ranks in one sweep.  A counting
//    pass is at most RPNET_VOLLOAD_SELECT_BLOCKS blocks that stride over the array; a wave whose active lanes all hold the same digit (the
//    air of a CT volume) adds its population with one LDS atomic instead of 64 serialised ones.  The pick is one block of 256 threads.
//    Four 4-byte read passes, 16 B per value.
//  - normalize: one launch, 16 bytes per lane, 8 B per value.  The file is built with -ffp-contract=off and every operation is spelled
//    with a rounding intrinsic, so neither the lerp nor `* 2 - 1` becomes an FMA; the division is __fdiv_rn under
//    -fhip-fp32-correctly-rounded-divide-sqrt.
//
// Bounds: a lane reads and writes only indices below the element count it was launched with (whole 16-byte accesses only where the run is
// whole and aligned); a gather reads a source index only after (z, y, x) has been placed inside the window, which the host has placed
// inside the volume.  Every loop runs to a count fixed when it is entered.
#include <climits>
#include <cmath>

#include "common.h"
#include "rpnet_volload_abi.h"

namespace rpnet {

constexpr int kVlBlocks = 8192;                      // blocks of a per-element sweep at most (range, gather, normalize)
constexpr size_t kVlHeadBytes = 64;
constexpr int kVlDigits = 256, kVlPasses = 4;
constexpr size_t kVlSelectBytes = kVlHeadBytes + (size_t)kVlPasses * 2 * kVlDigits * sizeof(unsigned);

struct VlHead {                                      // the first 64 bytes of a selection's workspace
    unsigned prefix[2];                              // the digits picked so far, most significant first
    unsigned rem[2];                                 // the rank among the keys that carry the prefix
    unsigned n_nan;
    unsigned pad[11];
};
static_assert(sizeof(VlHead) == kVlHeadBytes, "head layout");

static inline int vl_sweep_blocks(size_t lanes, int cap) { return (int)std::min<size_t>((lanes + 255) / 256, (size_t)cap); }
static inline int vl_sweep_iters(size_t lanes, int blocks) { return (int)((lanes + (size_t)blocks * 256 - 1) / ((size_t)blocks * 256)); }
static inline size_t vl_elem(int kind) { return kind == RPNET_PREP_F32 ? 4 : kind == RPNET_PREP_I16 ? 2 : 1; }

struct VlWindow {                                    // the window of truncate_image and the extents of pad2factor
    int nz, y1, tH, x1, tW, pH, pW;
};
static inline VlWindow vl_window(int D, int H, int W, int num_slice, int num_y, int num_x) {
    VlWindow w;
    w.nz = std::min(D, num_slice);
    w.y1 = std::max(0, H / 2 - num_y / 2);
    w.tH = std::min(H, H / 2 + num_y / 2) - w.y1;
    w.x1 = std::max(0, W / 2 - num_x / 2);
    w.tW = std::min(W, W / 2 + num_x / 2) - w.x1;
    w.pH = (w.tH + 15) / 16 * 16;
    w.pW = (w.tW + 15) / 16 * 16;
    return w;
}

// ------------------------------------------------------------------------------------------------------------------- range
static __global__ void vl_range_open_kernel(int32_t* __restrict__ row) {
    if (threadIdx.x == 0) {
        row[0] = INT_MAX;
        row[1] = -1;
        row[2] = 0;
        row[3] = 0;
    }
}

static __global__ void vl_range_close_kernel(int32_t* __restrict__ row) {
    if (threadIdx.x == 0 && row[0] == INT_MAX) row[0] = -1;
}

template <class T>
__device__ __forceinline__ bool vl_nonzero(const T v) { return v != (T)0; }       // float: true for a NaN

// lanes over runs of 16 bytes of the flat mask; a lane is (block * iters + it) * 256 + thread
template <class T>
__global__ __launch_bounds__(256) void vl_range_kernel(const T* __restrict__ mask, const unsigned n, const unsigned n_lanes, const int iters,
                                                       const int layout, const unsigned D, const unsigned H, const unsigned W, const VlWindow win,
                                                       int32_t* __restrict__ row) {
    RPNET_PASS_PRIORITY();
    constexpr unsigned R = 16 / sizeof(T);
    __shared__ int s_first, s_last;
    __shared__ unsigned s_count;
    const unsigned t = threadIdx.x;
    if (t == 0) {
        s_first = INT_MAX;
        s_last = -1;
        s_count = 0u;
    }
    __syncthreads();
    int first = INT_MAX, last = -1;
    unsigned count = 0u;
    for (int it = 0; it < iters; ++it) {
        const unsigned lane = ((unsigned)blockIdx.x * iters + it) * 256u + t;
        if (lane >= n_lanes) continue;
        const unsigned base = lane * R;
        const unsigned cnt = min(R, n - base);
        T e[R];
        if (cnt == R && ((uintptr_t)(mask + base) & 15u) == 0) {
            const uint4 w = *reinterpret_cast<const uint4*>(mask + base);
            __builtin_memcpy(e, &w, 16);
        } else {
#pragma unroll
            for (unsigned j = 0; j < R; ++j) e[j] = j < cnt ? mask[base + j] : (T)0;
        }
#pragma unroll
        for (unsigned j = 0; j < R; ++j) {
            if (!vl_nonzero(e[j])) continue;
            const unsigned i = base + j;
            unsigned z, y, x;
            if (layout == RPNET_VOLLOAD_X_FASTEST) {
                x = i % W;
                y = (i / W) % H;
                z = i / (W * H);
            } else {
                z = i % D;
                y = (i / D) % H;
                x = i / (D * H);
            }
            if ((int)z < win.nz && (int)y >= win.y1 && (int)y < win.y1 + win.tH && (int)x >= win.x1 && (int)x < win.x1 + win.tW) {
                first = min(first, (int)z);
                last = max(last, (int)z);
                ++count;
            }
        }
    }
    if (count) {
        atomicMin(&s_first, first);
        atomicMax(&s_last, last);
        atomicAdd(&s_count, count);
    }
    __syncthreads();
    if (t == 0 && s_count) {
        atomicMin(row + 0, s_first);
        atomicMax(row + 1, s_last);
        atomicAdd(row + 2, (int)s_count);
    }
}

// ------------------------------------------------------------------------------------------------------------------ gather
struct VlGather {
    int D, H, W, layout;                             // of the source
    VlWindow win;
    int lo, dn, ch, cw;
    int rh, cy, pt, rw, cx, pl;
    float pad;
};

template <class T>
__device__ __forceinline__ float vl_fetch(const T* __restrict__ src, const VlGather& g, const int d, const int oy, const int ox) {
    const int ry = oy - g.pt, rx = ox - g.pl;
    if (ry < 0 || ry >= g.rh || rx < 0 || rx >= g.rw) return g.pad;
    const int py = ry + g.cy, px = rx + g.cx;
    if (py >= g.win.tH || px >= g.win.tW) return g.pad;
    const size_t z = (size_t)(g.lo + d), y = (size_t)(g.win.y1 + py), x = (size_t)(g.win.x1 + px);
    const size_t i = g.layout == RPNET_VOLLOAD_X_FASTEST ? (z * g.H + y) * g.W + x : z + (size_t)g.D * (y + (size_t)g.H * x);
    return (float)src[i];
}

// lanes over (d, oy, run of 4 ox), runs fastest: n_lanes = dn * ch * ceil(cw / 4) < 2^30
template <class T>
__global__ __launch_bounds__(256) void vl_gather_kernel(const T* __restrict__ src, float* __restrict__ out, const VlGather g, const FastDiv div_runs,
                                                        const FastDiv div_ch, const unsigned n_lanes, const int iters) {
    RPNET_PASS_PRIORITY();
    for (int it = 0; it < iters; ++it) {
        const unsigned lane = ((unsigned)blockIdx.x * iters + it) * 256u + threadIdx.x;
        if (lane >= n_lanes) continue;
        unsigned q, d;
        const int ox = (int)div_runs.divmod(lane, q) * 4;
        const int oy = (int)div_ch.divmod(q, d);
        const int cnt = min(4, g.cw - ox);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? vl_fetch(src, g, (int)d, oy, ox + j) : 0.0f;
        float* p = out + ((size_t)d * g.ch + oy) * g.cw + ox;
        if (cnt == 4 && ((uintptr_t)p & 15u) == 0) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) p[j] = v[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ select
__device__ __forceinline__ unsigned vl_key(const float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;          // a NaN of either sign: behind +inf
    if (u == 0x80000000u) u = 0u;                                     // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vl_unkey(const unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// h[digit] += 1 for the lanes that are `on`: one atomic for the wave where all of them hold one digit.  Called by whole waves.
__device__ __forceinline__ void vl_hist_add(unsigned* h, const bool on, const unsigned digit, const int lane) {
    const unsigned long long m = __ballot(on);
    if (m == 0ull) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const unsigned d0 = (unsigned)__shfl((int)digit, lead);
    const unsigned long long same = __ballot(on && digit == d0);
    if (same == m) {
        if (lane == lead) atomicAdd(h + d0, (unsigned)__popcll(m));
    } else if (on) {
        atomicAdd(h + digit, 1u);
    }
}

static __global__ __launch_bounds__(256) void vl_select_open_kernel(unsigned* __restrict__ ws, const unsigned words, const unsigned k0,
                                                                    const unsigned k1) {
    for (unsigned i = threadIdx.x; i < words; i += 256u) ws[i] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        VlHead* head = reinterpret_cast<VlHead*>(ws);
        head->rem[0] = k0;
        head->rem[1] = k1;
    }
}

// pass kPass counts digit kPass (0 the most significant) of the keys whose higher digits are the rank's prefix; pass 0 counts the NaNs
template <int kPass>
__global__ __launch_bounds__(256) void vl_count_kernel(const float* __restrict__ x, const unsigned n, const unsigned n_lanes, const int iters,
                                                       VlHead* head, unsigned* __restrict__ hist) {
    RPNET_PASS_PRIORITY();
    constexpr int kShift = 24 - 8 * kPass;
    __shared__ unsigned h[2][kVlDigits];
    __shared__ unsigned s_nan;
    const unsigned t = threadIdx.x;
    const int lane_id = (int)(t & 63u);
    h[0][t] = 0u;
    h[1][t] = 0u;
    if (t == 0) s_nan = 0u;
    const unsigned p0 = kPass ? head->prefix[0] : 0u, p1 = kPass ? head->prefix[1] : 0u;
    const bool two = p0 != p1;                                        // uniform: the ranks have parted
    __syncthreads();
    unsigned nan = 0u;
    for (int it = 0; it < iters; ++it) {
        const unsigned lane = ((unsigned)blockIdx.x * iters + it) * 256u + t;
        const unsigned base = lane * 4u;                              // n_lanes * 4 < 2^31
        const unsigned cnt = lane < n_lanes ? min(4u, n - base) : 0u;
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (cnt == 4u && ((uintptr_t)(x + base) & 15u) == 0) {
            const float4 w = *reinterpret_cast<const float4*>(x + base);
            e[0] = w.x, e[1] = w.y, e[2] = w.z, e[3] = w.w;
        } else {
#pragma unroll
            for (unsigned j = 0; j < 4u; ++j)
                if (j < cnt) e[j] = x[base + j];
        }
#pragma unroll
        for (unsigned j = 0; j < 4u; ++j) {
            const bool valid = j < cnt;
            const unsigned key = vl_key(e[j]);
            const unsigned digit = (key >> kShift) & 255u;
            const unsigned above = kPass ? key >> (kShift + 8) : 0u;
            if (kPass == 0 && valid && key == 0xFFFFFFFFu) ++nan;
            vl_hist_add(h[0], valid && above == p0, digit, lane_id);
            if (two) vl_hist_add(h[1], valid && above == p1, digit, lane_id);
        }
    }
    if (kPass == 0 && nan) atomicAdd(&s_nan, nan);
    __syncthreads();
    unsigned* g = hist + (size_t)kPass * 2 * kVlDigits;
    if (h[0][t]) atomicAdd(g + t, h[0][t]);
    if (two && h[1][t]) atomicAdd(g + kVlDigits + t, h[1][t]);
    if (kPass == 0 && t == 0 && s_nan) atomicAdd(&head->n_nan, s_nan);
}

// one block: the digit of pass kPass in which each rank falls; after the last pass the two values and the NaN count
template <int kPass>
__global__ __launch_bounds__(256) void vl_pick_kernel(VlHead* __restrict__ head, const unsigned* __restrict__ hist, unsigned* __restrict__ stats) {
    __shared__ unsigned h[2][kVlDigits];
    const unsigned t = threadIdx.x;
    const unsigned* g = hist + (size_t)kPass * 2 * kVlDigits;
    const bool two = kPass && head->prefix[0] != head->prefix[1];
    h[0][t] = g[t];
    h[1][t] = two ? g[kVlDigits + t] : g[t];
    __syncthreads();
    if (t < 2) {
        unsigned rem = head->rem[t], digit = kVlDigits - 1, before = 0u;
        bool found = false;
        for (int d = 0; d < kVlDigits; ++d) {
            const unsigned c = h[t][d];
            if (!found && rem < before + c) {
                digit = (unsigned)d;
                rem -= before;
                found = true;
            }
            if (!found) before += c;
        }
        const unsigned prefix = ((kPass ? head->prefix[t] : 0u) << 8) | digit;
        head->prefix[t] = prefix;
        head->rem[t] = found ? rem : 0u;
        if (kPass == kVlPasses - 1) stats[t] = __float_as_uint(vl_unkey(prefix));
    }
    if (kPass == kVlPasses - 1 && t == 2) {
        stats[2] = head->n_nan;
        stats[3] = 0u;
    }
}

// --------------------------------------------------------------------------------------------------------------- normalize
__device__ __forceinline__ float vl_map(float v, const float top, const float mn, const float mx, const float den) {
    if (v > top) v = top;
    if (v > mx) v = mx;
    if (v < mn) v = mn;
    return __fsub_rn(__fmul_rn(__fdiv_rn(__fsub_rn(v, mn), den), 2.0f), 1.0f);
}

__global__ __launch_bounds__(256) void vl_normalize_kernel(const float* in, float* out, const size_t n, const size_t n_lanes, const int iters,
                                                           const unsigned* __restrict__ stats, const float g, const float mn, const float mx,
                                                           const float den) {
    RPNET_PASS_PRIORITY();
    const float a = __uint_as_float(stats[0]), b = __uint_as_float(stats[1]);
    const float diff = __fsub_rn(b, a);
    float top = g >= 0.5f ? __fsub_rn(b, __fmul_rn(diff, __fsub_rn(1.0f, g))) : __fadd_rn(a, __fmul_rn(diff, g));
    if (stats[2] != 0u) top = __uint_as_float(0x7FC00000u);
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)blockIdx.x * iters + it) * 256u + threadIdx.x;
        if (lane >= n_lanes) continue;
        const size_t base = lane * 4u;
        const int cnt = (int)std::min<size_t>((size_t)4, n - base);
        if (cnt == 4 && (((uintptr_t)(in + base) | (uintptr_t)(out + base)) & 15u) == 0) {
            float4 w = *reinterpret_cast<const float4*>(in + base);
            w.x = vl_map(w.x, top, mn, mx, den);
            w.y = vl_map(w.y, top, mn, mx, den);
            w.z = vl_map(w.z, top, mn, mx, den);
            w.w = vl_map(w.w, top, mn, mx, den);
            *reinterpret_cast<float4*>(out + base) = w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) out[base + j] = vl_map(in[base + j], top, mn, mx, den);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
static inline bool vl_dims_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= RPNET_CC_MAX_DIM && H <= RPNET_CC_MAX_DIM && W <= RPNET_CC_MAX_DIM;
}
static inline bool vl_kind_ok(int kind) { return kind == RPNET_PREP_F32 || kind == RPNET_PREP_I16 || kind == RPNET_VOLLOAD_U8; }

template <class T>
static void vl_range_launch(const void* mask, int layout, int D, int H, int W, const VlWindow& win, int32_t* row, hipStream_t st) {
    const size_t n = (size_t)D * H * W, n_lanes = (n * sizeof(T) + 15) / 16;
    const int blocks = vl_sweep_blocks(n_lanes, kVlBlocks), iters = vl_sweep_iters(n_lanes, blocks);
    hipLaunchKernelGGL(vl_range_kernel<T>, dim3(blocks), dim3(256), 0, st, static_cast<const T*>(mask), (unsigned)n, (unsigned)n_lanes, iters, layout,
                       (unsigned)D, (unsigned)H, (unsigned)W, win, row);
}

template <class T>
static void vl_gather_launch(const void* src, float* out, const VlGather& g, hipStream_t st) {
    const int runs = cdiv(g.cw, 4);
    const size_t n_lanes = (size_t)g.dn * g.ch * runs;
    const int blocks = vl_sweep_blocks(n_lanes, kVlBlocks), iters = vl_sweep_iters(n_lanes, blocks);
    hipLaunchKernelGGL(vl_gather_kernel<T>, dim3(blocks), dim3(256), 0, st, static_cast<const T*>(src), out, g, FastDiv((unsigned)runs),
                       FastDiv((unsigned)g.ch), (unsigned)n_lanes, iters);
}

template <int kPass>
static void vl_select_pass(const float* x, size_t n, VlHead* head, unsigned* hist, unsigned* stats, hipStream_t st) {
    const size_t n_lanes = (n + 3) / 4;
    const int blocks = vl_sweep_blocks(n_lanes, RPNET_VOLLOAD_SELECT_BLOCKS), iters = vl_sweep_iters(n_lanes, blocks);
    hipLaunchKernelGGL(vl_count_kernel<kPass>, dim3(blocks), dim3(256), 0, st, x, (unsigned)n, (unsigned)n_lanes, iters, head, hist);
    hipLaunchKernelGGL(vl_pick_kernel<kPass>, dim3(1), dim3(256), 0, st, head, hist, stats);
}

}  // namespace rpnet

extern "C" int rpnet_volload_abi_version(void) { return RPNET_VOLLOAD_ABI_VERSION; }

extern "C" size_t rpnet_volload_select_workspace_bytes(size_t n) {
    using namespace rpnet;
    if (n < 1 || n > (size_t)RPNET_VOLLOAD_MAX_N) {
        set_error("volload_select: n=%zu (1..%d values)", n, RPNET_VOLLOAD_MAX_N);
        return 0;
    }
    return kVlSelectBytes;
}

#define RPNET_VOLLOAD_SOURCE_CHECKS(p)                                                                                                               \
    RPNET_REQUIRE(vl_kind_ok(kind), RPNET_ERR_ARG, "%s: element kind %d (0 float32, 1 int16, 2 uint8)", fn, kind);                                  \
    RPNET_REQUIRE(layout == RPNET_VOLLOAD_X_FASTEST || layout == RPNET_VOLLOAD_Z_FASTEST, RPNET_ERR_ARG, "%s: layout %d (0 x fastest, 1 z fastest)", \
                  fn, layout);                                                                                                                       \
    RPNET_REQUIRE(vl_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);                  \
    RPNET_REQUIRE(num_slice >= 1 && num_y >= 1 && num_x >= 1, RPNET_ERR_ARG, "%s: num_slice=%d num_y=%d num_x=%d (each at least 1)", fn, num_slice,  \
                  num_y, num_x);                                                                                                                     \
    const VlWindow win = vl_window(D, H, W, num_slice, num_y, num_x);                                                                                \
    RPNET_REQUIRE(win.tH >= 1 && win.tW >= 1, RPNET_ERR_SHAPE, "%s: the window of num_y=%d num_x=%d in H=%d W=%d is empty", fn, num_y, num_x, H, W); \
    RPNET_REQUIRE(((uintptr_t)(p) % vl_elem(kind)) == 0, RPNET_ERR_ARG, "%s: the source must be aligned to its element", fn)

extern "C" int rpnet_volload_range(const void* mask, int kind, int layout, int D, int H, int W, int num_slice, int num_y, int num_x, int32_t* row,
                                   rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "volload_range";
    RPNET_REQUIRE(mask && row, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_VOLLOAD_SOURCE_CHECKS(mask);
    RPNET_REQUIRE(((uintptr_t)row % 16) == 0, RPNET_ERR_ARG, "%s: the row must be aligned to 16 bytes", fn);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vl_range_open_kernel, dim3(1), dim3(64), 0, st, row);
    if (kind == RPNET_PREP_F32) vl_range_launch<float>(mask, layout, D, H, W, win, row, st);
    else if (kind == RPNET_PREP_I16) vl_range_launch<int16_t>(mask, layout, D, H, W, win, row, st);
    else vl_range_launch<uint8_t>(mask, layout, D, H, W, win, row, st);
    hipLaunchKernelGGL(vl_range_close_kernel, dim3(1), dim3(64), 0, st, row);
    return check_launch(fn);
}

extern "C" int rpnet_volload_gather(const void* src, int kind, int layout, int D, int H, int W, int num_slice, int num_y, int num_x, int lo, int hi,
                                    int crop_h, int crop_w, float pad_value, float* out, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "volload_gather";
    RPNET_REQUIRE(src && out, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_VOLLOAD_SOURCE_CHECKS(src);
    RPNET_REQUIRE(lo >= 0 && lo < hi && hi <= win.nz, RPNET_ERR_ARG, "%s: lo=%d hi=%d (0 <= lo < hi <= %d)", fn, lo, hi, win.nz);
    RPNET_REQUIRE(crop_h >= 1 && crop_w >= 1 && crop_h <= RPNET_CC_MAX_DIM && crop_w <= RPNET_CC_MAX_DIM, RPNET_ERR_SHAPE,
                  "%s: crop_h=%d crop_w=%d (each 1..%d)", fn, crop_h, crop_w, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(((uintptr_t)out % 4) == 0, RPNET_ERR_ARG, "%s: out must be aligned to 4 bytes", fn);
    VlGather g;
    g.D = D, g.H = H, g.W = W, g.layout = layout, g.win = win;
    g.lo = lo, g.dn = hi - lo, g.ch = crop_h, g.cw = crop_w;
    g.rh = std::min(crop_h, win.pH), g.cy = win.pH / 2 - g.rh / 2, g.pt = (crop_h - g.rh) / 2;
    g.rw = std::min(crop_w, win.pW), g.cx = win.pW / 2 - g.rw / 2, g.pl = (crop_w - g.rw) / 2;
    g.pad = pad_value;
    hipStream_t st = (hipStream_t)stream;
    if (kind == RPNET_PREP_F32) vl_gather_launch<float>(src, out, g, st);
    else if (kind == RPNET_PREP_I16) vl_gather_launch<int16_t>(src, out, g, st);
    else vl_gather_launch<uint8_t>(src, out, g, st);
    return check_launch(fn);
}

extern "C" int rpnet_volload_select(const float* x, size_t n, size_t k0, size_t k1, void* stats, void* workspace, size_t workspace_bytes,
                                    rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "volload_select";
    RPNET_REQUIRE(x && stats && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(n >= 1 && n <= (size_t)RPNET_VOLLOAD_MAX_N, RPNET_ERR_SHAPE, "%s: n=%zu (1..%d values)", fn, n, RPNET_VOLLOAD_MAX_N);
    RPNET_REQUIRE(k0 <= k1 && k1 <= n - 1, RPNET_ERR_ARG, "%s: ranks %zu, %zu of %zu values (k0 <= k1 <= n - 1)", fn, k0, k1, n);
    RPNET_REQUIRE(workspace_bytes >= kVlSelectBytes, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes,
                  kVlSelectBytes);
    RPNET_REQUIRE(((uintptr_t)x % 4) == 0 && ((uintptr_t)stats % 16) == 0 && ((uintptr_t)workspace % 16) == 0, RPNET_ERR_ARG,
                  "%s: x must be aligned to 4 bytes, stats and the workspace to 16", fn);
    hipStream_t st = (hipStream_t)stream;
    unsigned* ws = static_cast<unsigned*>(workspace);
    VlHead* head = reinterpret_cast<VlHead*>(ws);
    unsigned* hist = ws + kVlHeadBytes / sizeof(unsigned);
    hipLaunchKernelGGL(vl_select_open_kernel, dim3(1), dim3(256), 0, st, ws, (unsigned)(kVlSelectBytes / sizeof(unsigned)), (unsigned)k0, (unsigned)k1);
    vl_select_pass<0>(x, n, head, hist, static_cast<unsigned*>(stats), st);
    vl_select_pass<1>(x, n, head, hist, static_cast<unsigned*>(stats), st);
    vl_select_pass<2>(x, n, head, hist, static_cast<unsigned*>(stats), st);
    vl_select_pass<3>(x, n, head, hist, static_cast<unsigned*>(stats), st);
    return check_launch(fn);
}

extern "C" int rpnet_volload_normalize(const float* in, float* out, size_t n, const void* stats, float g, float minimum, float maximum,
                                       float denominator, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "volload_normalize";
    RPNET_REQUIRE(in && out && stats, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(n >= 1 && n <= (size_t)RPNET_VOLLOAD_MAX_N, RPNET_ERR_SHAPE, "%s: n=%zu (1..%d values)", fn, n, RPNET_VOLLOAD_MAX_N);
    RPNET_REQUIRE(((uintptr_t)in % 4) == 0 && ((uintptr_t)out % 4) == 0 && ((uintptr_t)stats % 16) == 0, RPNET_ERR_ARG,
                  "%s: in and out must be aligned to 4 bytes, stats to 16", fn);
    const uintptr_t a0 = (uintptr_t)in, b0 = (uintptr_t)out;
    RPNET_REQUIRE(a0 == b0 || a0 + 4 * n <= b0 || b0 + 4 * n <= a0, RPNET_ERR_ARG, "%s: out partly overlaps in", fn);
    RPNET_REQUIRE(minimum <= maximum && denominator >= 1.0f && g >= 0.0f && g < 1.0f, RPNET_ERR_ARG,
                  "%s: minimum=%g maximum=%g denominator=%g g=%g (minimum <= maximum, denominator >= 1, 0 <= g < 1)", fn, (double)minimum,
                  (double)maximum, (double)denominator, (double)g);
    const size_t n_lanes = (n + 3) / 4;
    const int blocks = vl_sweep_blocks(n_lanes, kVlBlocks), iters = vl_sweep_iters(n_lanes, blocks);
    hipLaunchKernelGGL(vl_normalize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, in, out, n, n_lanes, iters,
                       static_cast<const unsigned*>(stats), g, minimum, maximum, denominator);
    return check_launch(fn);
}
