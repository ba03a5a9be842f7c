// Resampling of a [D][H][W] image or label map to a grid of another shape, trilinear or nearest neighbour (include/rpnet_resample_abi.h;
// rpnet_amd/resample.py): the `resample(image, spacing, new_spacing)` stage of the reference's preprocessing, on the device.
//
// What was chosen.  The work is a gather bound by memory, so the coordinates are not redone per voxel: one small launch writes, for every
// output index of the three axes, a 16-byte entry {i0, i1, t} (or the nearest index) into the workspace, and the gather reads three of
// them per voxel from cache.  A lane of the gather owns a run of 16 bytes of consecutive output x positions of one output row (4 float32,
// 8 int16, 16 uint8): the z and y entries and the four input row pointers are formed once per run, the x entries are consecutive 16-byte
// loads, and the run leaves as one 16-byte store where it is whole and its address 16-byte aligned (decided per lane, so an odd row
// length only costs the lanes it misaligns).  Neighbouring lanes own neighbouring runs, so a wave writes 1 KiB of a row at a time and
// its taps fall in a few input rows.
// The float64 operations of the definition are spelled one rounding at a time and the file is built with -ffp-contract=off: a numpy
// restatement gets the same bits.  A tap of weight zero is loaded (its index is in range by construction) but not used.
//
// Bounds: every index of a table is clamped to its axis when the table is written (0 <= i0 <= i1 <= n - 1); a lane beyond the last run
// does nothing; a run reads the x entries min(x, Wo - 1) and stores only its `cnt` elements.  Every loop runs to a count fixed when it
// is entered.  The counts of the statistics row go through LDS and one integer atomic per block.
#include <cmath>

#include "cc_phases.h"
#include "rpnet_resample_abi.h"

namespace rpnet {

struct ResampleEntry {                              // one output index of one axis
    int i0, i1;                                     // NEAREST: i0 is the nearest index, i1 = 0
    double t;
};
struct ResampleHead {                               // the 64 bytes in front of the tables
    unsigned long long n_in, n_out, spare[6];
};
static_assert(sizeof(ResampleEntry) == 16 && sizeof(ResampleHead) == kCcHeadBytes, "workspace layout of the header");

constexpr int kResampleRunBytes = 16;               // bytes of the run of a lane
constexpr int kNearest = 0, kLinear = 1, kIndicator = 2;    // what the gather does with its taps

// lerp of the definition: a tap of weight zero is not used
__device__ __forceinline__ double resample_lerp(const double a, const double b, const double t) {
    return t == 0.0 ? a : __dadd_rn(a, __dmul_rn(t, __dsub_rn(b, a)));
}

// the one conversion of a result to the output kind
__device__ __forceinline__ float resample_convert(const double r, float) { return (float)r; }
__device__ __forceinline__ int16_t resample_convert(const double r, int16_t) {
    return (int16_t)(int)fmin(fmax(rint(r), -32768.0), 32767.0);              // rint: half to even
}

// ------------------------------------------------------------------------------------------------------------------ tables
// tab: Do + Ho + Wo entries, z then y then x.  grid ceil((Do + Ho + Wo) / 256)
__global__ __launch_bounds__(256) void resample_tables_kernel(ResampleHead* __restrict__ head, ResampleEntry* __restrict__ tab, const int Di,
                                                              const int Hi, const int Wi, const int Do, const int Ho, const int Wo,
                                                              const int center, const int linear) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < kCcHeadBytes / sizeof(unsigned long long)) reinterpret_cast<unsigned long long*>(head)[threadIdx.x] = 0ull;
    if (i >= Do + Ho + Wo) return;
    const int n = i < Do ? Di : (i < Do + Ho ? Hi : Wi), m = i < Do ? Do : (i < Do + Ho ? Ho : Wo);
    const int o = i < Do ? i : (i < Do + Ho ? i - Do : i - Do - Ho);
    double c;
    if (center) {
        c = __dsub_rn(__ddiv_rn((double)((2 * o + 1) * n), (double)(2 * m)), 0.5);  // (2o + 1) n < 2^21
        c = fmin(fmax(c, 0.0), (double)(n - 1));
    } else {
        c = m == 1 ? 0.0 : __ddiv_rn((double)(o * (n - 1)), (double)(m - 1));
    }
    ResampleEntry e;
    if (linear) {
        e.i0 = min((int)floor(c), n - 1);
        e.i1 = min(e.i0 + 1, n - 1);
        e.t = __dsub_rn(c, (double)e.i0);
    } else {
        e.i0 = min(max((int)floor(__dadd_rn(c, 0.5)), 0), n - 1);
        e.i1 = 0;
        e.t = 0.0;
    }
    tab[i] = e;
}

// ------------------------------------------------------------------------------------------------------------------- count
// the input voxels equal to cls: 16 per lane over the flat volume, a 16-byte load where the lane is whole and aligned
__global__ __launch_bounds__(256) void resample_count_kernel(const uint8_t* __restrict__ in, const size_t n, const size_t n_lanes, const int iters,
                                                             const int cls, ResampleHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned s;
    const int t = threadIdx.x;
    if (t == 0) s = 0u;
    __syncthreads();
    unsigned cnt_cls = 0u;
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)blockIdx.x * iters + it) * 256u + t;
        if (lane >= n_lanes) continue;
        const size_t base = lane * 16u;
        const int cnt = (int)std::min<size_t>((size_t)16, n - base);
        const uint8_t* q = in + base;
        uint8_t v[16];
        if (cnt == 16 && ((uintptr_t)q & 15u) == 0) {
            const uint4 w = *reinterpret_cast<const uint4*>(q);
            __builtin_memcpy(v, &w, 16);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = j < cnt ? q[j] : (uint8_t)0;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) cnt_cls += j < cnt && (int)v[j] == cls;
    }
    if (cnt_cls) atomicAdd(&s, cnt_cls);
    __syncthreads();
    if (t == 0 && s) atomicAdd(&head->n_in, (unsigned long long)s);
}

// ------------------------------------------------------------------------------------------------------------------ gather
// lanes over (output row, run of the row): lpr runs per row, n_lanes = Do * Ho * lpr < 2^28.  tz, ty, tx: the tables of the three axes.
// kMode: kNearest copies the voxel, kLinear is the image rule, kIndicator the label rule of class cls (T = uint8_t; merge reads out).
template <class T, int kMode>
__global__ __launch_bounds__(256) void resample_gather_kernel(const T* __restrict__ in, T* out, const int Hi, const int Wi, const int Ho, const int Wo,
                                                              const FastDiv div_lpr, const FastDiv div_ho, const unsigned n_lanes, const int iters,
                                                              const ResampleEntry* __restrict__ tz, const ResampleEntry* __restrict__ ty,
                                                              const ResampleEntry* __restrict__ tx, const int cls, const int merge, const int count,
                                                              ResampleHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    constexpr int R = kResampleRunBytes / (int)sizeof(T);
    __shared__ unsigned s;
    const int t = threadIdx.x;
    if (t == 0) s = 0u;
    __syncthreads();
    unsigned n_cls = 0u;
    for (int it = 0; it < iters; ++it) {
        const unsigned lane = ((unsigned)blockIdx.x * iters + it) * 256u + t;
        if (lane >= n_lanes) continue;
        unsigned row, z;
        const int x0 = (int)div_lpr.divmod(lane, row) * R;
        const int y = (int)div_ho.divmod(row, z);
        const int cnt = min(R, Wo - x0);
        const ResampleEntry ez = tz[z], ey = ty[y];
        const T* p00 = in + ((size_t)ez.i0 * Hi + ey.i0) * Wi;
        T* q = out + (size_t)row * Wo + x0;
        const bool whole = cnt == R && ((uintptr_t)q & 15u) == 0;
        T o[R];
        if (kMode == kIndicator && merge) {        // what the output holds: it keeps every value but 0
            if (whole) {
                const uint4 w = *reinterpret_cast<const uint4*>(q);
                __builtin_memcpy(o, &w, 16);
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j) o[j] = j < cnt ? q[j] : (T)0;
            }
        }
        if constexpr (kMode == kNearest) {
#pragma unroll
            for (int j = 0; j < R; ++j) o[j] = p00[tx[min(x0 + j, Wo - 1)].i0];
        } else {
            const T* p01 = in + ((size_t)ez.i0 * Hi + ey.i1) * Wi;
            const T* p10 = in + ((size_t)ez.i1 * Hi + ey.i0) * Wi;
            const T* p11 = in + ((size_t)ez.i1 * Hi + ey.i1) * Wi;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const ResampleEntry ex = tx[min(x0 + j, Wo - 1)];
                double a[8];
                const T raw[8] = {p00[ex.i0], p00[ex.i1], p01[ex.i0], p01[ex.i1], p10[ex.i0], p10[ex.i1], p11[ex.i0], p11[ex.i1]};
#pragma unroll
                for (int k = 0; k < 8; ++k) a[k] = kMode == kIndicator ? ((int)raw[k] == cls ? 1.0 : 0.0) : (double)raw[k];
                const double v00 = resample_lerp(a[0], a[1], ex.t), v01 = resample_lerp(a[2], a[3], ex.t);
                const double v10 = resample_lerp(a[4], a[5], ex.t), v11 = resample_lerp(a[6], a[7], ex.t);
                const double r = resample_lerp(resample_lerp(v00, v01, ey.t), resample_lerp(v10, v11, ey.t), ez.t);
                if constexpr (kMode == kIndicator) {
                    const bool hit = r > 0.5;
                    o[j] = merge ? ((hit && o[j] == (T)0) ? (T)cls : o[j]) : (hit ? (T)cls : (T)0);
                } else {
                    o[j] = resample_convert(r, T());
                }
            }
        }
        if constexpr (sizeof(T) == 1) {
            if (count) {
#pragma unroll
                for (int j = 0; j < R; ++j) n_cls += j < cnt && (int)o[j] == cls;
            }
        }
        if (whole) {
            uint4 w;
            __builtin_memcpy(&w, o, 16);
            *reinterpret_cast<uint4*>(q) = w;
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (j < cnt) q[j] = o[j];
        }
    }
    if (n_cls) atomicAdd(&s, n_cls);
    __syncthreads();
    if (t == 0 && s) atomicAdd(&head->n_out, (unsigned long long)s);
}

__global__ __launch_bounds__(64) void resample_stats_row_kernel(const ResampleHead* __restrict__ head, const long long total, long long* __restrict__ row) {
    if (threadIdx.x != 0) return;
    row[0] = (long long)head->n_in;
    row[1] = (long long)head->n_out;
    row[2] = total;
    row[3] = 0ll;
}

// ------------------------------------------------------------------------------------------------------------------- host
static inline size_t resample_need(int Do, int Ho, int Wo) { return kCcHeadBytes + sizeof(ResampleEntry) * ((size_t)Do + Ho + Wo); }
static inline bool resample_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}
static inline bool resample_align_ok(int align) { return align == RPNET_RESAMPLE_CORNER || align == RPNET_RESAMPLE_CENTER; }
static inline bool resample_order_ok(int order) { return order == RPNET_RESAMPLE_NEAREST || order == RPNET_RESAMPLE_LINEAR; }

static void resample_tables(void* ws, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int align, bool linear, hipStream_t st) {
    char* p = static_cast<char*>(ws);
    hipLaunchKernelGGL(resample_tables_kernel, dim3(cdiv(Do + Ho + Wo, 256)), dim3(256), 0, st, reinterpret_cast<ResampleHead*>(p),
                       reinterpret_cast<ResampleEntry*>(p + kCcHeadBytes), Di, Hi, Wi, Do, Ho, Wo, align == RPNET_RESAMPLE_CENTER ? 1 : 0, linear ? 1 : 0);
}

template <class T, int kMode>
static void resample_gather(const void* in, void* out, int Hi, int Wi, int Do, int Ho, int Wo, int cls, int merge, bool count, void* ws, hipStream_t st) {
    constexpr int R = kResampleRunBytes / (int)sizeof(T);
    const int lpr = cdiv(Wo, R);
    const size_t n_lanes = (size_t)Do * Ho * lpr;                               // <= 2^20 * 256
    const int blocks = cc_sweep_blocks(n_lanes), iters = cc_sweep_iters(n_lanes, blocks);
    char* p = static_cast<char*>(ws);
    const ResampleEntry* tab = reinterpret_cast<const ResampleEntry*>(p + kCcHeadBytes);
    hipLaunchKernelGGL((resample_gather_kernel<T, kMode>), dim3(blocks), dim3(256), 0, st, static_cast<const T*>(in), static_cast<T*>(out), Hi, Wi, Ho, Wo,
                       FastDiv((unsigned)lpr), FastDiv((unsigned)Ho), (unsigned)n_lanes, iters, tab, tab + Do, tab + Do + Ho, cls, merge, count ? 1 : 0,
                       reinterpret_cast<ResampleHead*>(p));
}

}  // namespace rpnet

extern "C" int rpnet_resample_abi_version(void) { return RPNET_RESAMPLE_ABI_VERSION; }

extern "C" size_t rpnet_resample_workspace_bytes(int Di, int Hi, int Wi, int Do, int Ho, int Wo) {
    using namespace rpnet;
    if (!cc_dims_ok(Di, Hi, Wi) || !cc_dims_ok(Do, Ho, Wo)) {
        set_error("resample: D=%d H=%d W=%d -> D=%d H=%d W=%d (every extent 1..%d)", Di, Hi, Wi, Do, Ho, Wo, RPNET_CC_MAX_DIM);
        return 0;
    }
    return resample_need(Do, Ho, Wo);
}

#define RPNET_RESAMPLE_COMMON_CHECKS(fn)                                                                                                   \
    RPNET_REQUIRE(cc_dims_ok(Di, Hi, Wi) && cc_dims_ok(Do, Ho, Wo), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d -> D=%d H=%d W=%d (every extent 1..%d)", \
                  fn, Di, Hi, Wi, Do, Ho, Wo, RPNET_CC_MAX_DIM);                                                                           \
    RPNET_REQUIRE(resample_align_ok(align), RPNET_ERR_ARG, "%s: align %d (0 corner, 1 center)", fn, align);                                \
    const size_t need = resample_need(Do, Ho, Wo);                                                                                         \
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need)

extern "C" int rpnet_resample_image(const void* in, int kind, int Di, int Hi, int Wi, void* out, int Do, int Ho, int Wo, int align, int order,
                                    void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "resample_image";
    RPNET_REQUIRE(in && out && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(kind == RPNET_PREP_F32 || kind == RPNET_PREP_I16, RPNET_ERR_ARG, "%s: element kind %d (0 float32, 1 int16)", fn, kind);
    RPNET_REQUIRE(resample_order_ok(order), RPNET_ERR_ARG, "%s: order %d (0 nearest, 1 linear)", fn, order);
    RPNET_RESAMPLE_COMMON_CHECKS(fn);
    const size_t es = kind == RPNET_PREP_F32 ? 4 : 2, n_in = (size_t)Di * Hi * Wi * es, n_out = (size_t)Do * Ho * Wo * es;
    RPNET_REQUIRE(((uintptr_t)in % es) == 0 && ((uintptr_t)out % es) == 0 && ((uintptr_t)workspace % 16) == 0, RPNET_ERR_ARG,
                  "%s: the volumes must be aligned to their element and the workspace to 16 bytes", fn);
    RPNET_REQUIRE(resample_disjoint(in, n_in, out, n_out), RPNET_ERR_ARG, "%s: out overlaps in", fn);
    hipStream_t st = (hipStream_t)stream;
    const bool linear = order == RPNET_RESAMPLE_LINEAR;
    resample_tables(workspace, Di, Hi, Wi, Do, Ho, Wo, align, linear, st);
    if (kind == RPNET_PREP_F32) {
        if (linear) resample_gather<float, kLinear>(in, out, Hi, Wi, Do, Ho, Wo, 0, 0, false, workspace, st);
        else resample_gather<float, kNearest>(in, out, Hi, Wi, Do, Ho, Wo, 0, 0, false, workspace, st);
    } else {
        if (linear) resample_gather<int16_t, kLinear>(in, out, Hi, Wi, Do, Ho, Wo, 0, 0, false, workspace, st);
        else resample_gather<int16_t, kNearest>(in, out, Hi, Wi, Do, Ho, Wo, 0, 0, false, workspace, st);
    }
    return check_launch(fn);
}

extern "C" int rpnet_resample_labels(const uint8_t* in, int Di, int Hi, int Wi, uint8_t* out, int Do, int Ho, int Wo, int cls, int align, int mode,
                                     int merge, int64_t* stats, int64_t row, int64_t rows, void* workspace, size_t workspace_bytes,
                                     rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "resample_labels";
    RPNET_REQUIRE(in && out && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(resample_order_ok(mode), RPNET_ERR_ARG, "%s: mode %d (0 nearest, 1 linear)", fn, mode);
    const bool linear = mode == RPNET_RESAMPLE_LINEAR;
    RPNET_REQUIRE(cls >= (linear ? 1 : 0) && cls <= 255, RPNET_ERR_ARG, "%s: class %d (%d..255: the volumes are uint8)", fn, cls, linear ? 1 : 0);
    RPNET_REQUIRE(!linear || merge == 0 || merge == 1, RPNET_ERR_ARG, "%s: merge %d (0 or 1)", fn, merge);
    RPNET_RESAMPLE_COMMON_CHECKS(fn);
    RPNET_REQUIRE(!stats || (rows >= 1 && row >= 0 && row < rows), RPNET_ERR_ARG, "%s: row %lld of a table of %lld rows", fn, (long long)row,
                  (long long)rows);
    RPNET_REQUIRE(((uintptr_t)stats % 8) == 0 && ((uintptr_t)workspace % 16) == 0, RPNET_ERR_ARG,
                  "%s: the table must be aligned to 8 and the workspace to 16 bytes", fn);
    const size_t n_in = (size_t)Di * Hi * Wi, n_out = (size_t)Do * Ho * Wo;
    RPNET_REQUIRE(resample_disjoint(in, n_in, out, n_out), RPNET_ERR_ARG, "%s: out overlaps in", fn);
    hipStream_t st = (hipStream_t)stream;
    resample_tables(workspace, Di, Hi, Wi, Do, Ho, Wo, align, linear, st);
    ResampleHead* head = static_cast<ResampleHead*>(workspace);
    if (stats) {
        const size_t n_lanes = (n_in + 15) / 16;
        const int blocks = cc_sweep_blocks(n_lanes);
        hipLaunchKernelGGL(resample_count_kernel, dim3(blocks), dim3(256), 0, st, in, n_in, n_lanes, cc_sweep_iters(n_lanes, blocks), cls, head);
    }
    if (linear) resample_gather<uint8_t, kIndicator>(in, out, Hi, Wi, Do, Ho, Wo, cls, merge, stats != nullptr, workspace, st);
    else resample_gather<uint8_t, kNearest>(in, out, Hi, Wi, Do, Ho, Wo, cls, 0, stats != nullptr, workspace, st);
    if (stats)
        hipLaunchKernelGGL(resample_stats_row_kernel, dim3(1), dim3(64), 0, st, head, (long long)n_out,
                           reinterpret_cast<long long*>(stats + row * RPNET_RESAMPLE_STATS_ROW));
    return check_launch(fn);
}
