// Region statistics of a segmented volume (include/rpnet_region_abi.h): per label the voxel count, the bounding box, the first and
// second coordinate moments, and the float64 sums and the extrema of the image inside it, in one pass over the labels and the image.
//
// A block of 256 lanes owns a chunk of 4096 voxels, 16 consecutive ones per lane.  It marks the labels its chunk holds in a 256-bit
// mask in LDS (one atomicOr per wave where the whole wave holds one label, the common case in a real mask) and walks the set bits in
// ascending order: per present label the lanes form their partial sums, the geometry is folded by wave reductions in 32 bits (a wave
// holds 1024 voxels with coordinates below 1024, so every sum of a wave is below 2^30), the four waves are combined in 64 bits and
// added to the accumulators of the workspace by integer atomics, and the float64 sums go through the tree the header states.  A
// second launch folds the partials of the blocks and decodes the accumulators into the rows.
//
// Bounds: every loop runs to a count fixed when it is entered (the trips of a block, the 16 voxels of a lane, the set bits of a
// mask word, the partials of a thread).  Atomics are integer ones only, so their order does not reach the result.  No block waits
// for another; what the fold reads, the pass wrote in an earlier launch.
#include <algorithm>

#include "common.h"
#include "rpnet_region_abi.h"

namespace rpnet {
namespace {

typedef unsigned long long reg_u64;
constexpr int kRegLane = 16;                                    // voxels of a lane
constexpr int kRegCols = RPNET_REGION_IROW;
constexpr int kRegAccBytes = 8 * RPNET_REGION_IROW;             // of one label's accumulators

static inline bool reg_dims_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= RPNET_CC_MAX_DIM && H <= RPNET_CC_MAX_DIM && W <= RPNET_CC_MAX_DIM;
}
static inline size_t reg_chunks(int D, int H, int W) {
    return ((size_t)D * H * W + RPNET_REGION_CHUNK - 1) / RPNET_REGION_CHUNK;
}
static inline size_t reg_need(int D, int H, int W, int L) {
    const size_t G = std::min<size_t>(reg_chunks(D, H, W), RPNET_REGION_MAX_BLOCKS);
    return RPNET_REGION_HEAD_BYTES + (size_t)kRegAccBytes * L + 16 * G * L;
}

// the voxels of a lane: 16-byte accesses where the lane is whole and its first address aligned; v[j] = 0 beyond cnt
template <class T>
__device__ __forceinline__ void reg_load16(const T* p, const unsigned base, const int cnt, T (&v)[kRegLane]) {
    const T* q = p + base;
    if (cnt == kRegLane && ((uintptr_t)q & 15u) == 0) {
        constexpr int kWords = (int)sizeof(T);      // 16 elements are sizeof(T) words of 16 bytes
        uint4 w[kWords];
#pragma unroll
        for (int k = 0; k < kWords; ++k) w[k] = reinterpret_cast<const uint4*>(q)[k];
        __builtin_memcpy(v, w, sizeof(w));
    } else {
#pragma unroll
        for (int j = 0; j < kRegLane; ++j) v[j] = j < cnt ? q[j] : (T)0;
    }
}

// the label a value names, 0 .. L-1, or -1: outside
__device__ __forceinline__ int reg_label(const uint8_t v, const int L) { return (int)v < L ? (int)v : -1; }
__device__ __forceinline__ int reg_label(const int32_t v, const int L) { return (v >= 0 && v < L) ? v : -1; }
__device__ __forceinline__ int reg_label(const int64_t v, const int L) { return (v >= 0 && v < (int64_t)L) ? (int)v : -1; }
__device__ __forceinline__ int reg_label(const float v, const int L) {
    if (!(v >= 0.0f && v < (float)L)) return -1;            // a NaN fails both
    const int l = (int)v;
    return (float)l == v ? l : -1;
}

// the key of rpnet_volload_abi.h of a finite value
__device__ __forceinline__ unsigned reg_key(const float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned reg_wave_add(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned reg_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
    return v;
}

// The tree of the header over red[0][.] and red[1][.], which hold the 256 values of the lanes: the strides 128 and 64 in LDS, the
// strides 32 .. 1 inside wave 0, where lane t adds what lane t + s holds: the same additions in the same order.  The caller has
// synchronised after the writes; the results are valid in thread 0.
__device__ __forceinline__ void reg_tree(double (*red)[256], const int t, double& r1, double& r2) {
    if (t < 128) {
        red[0][t] = __dadd_rn(red[0][t], red[0][t + 128]);
        red[1][t] = __dadd_rn(red[1][t], red[1][t + 128]);
    }
    __syncthreads();
    if (t < 64) {
        r1 = __dadd_rn(red[0][t], red[0][t + 64]);
        r2 = __dadd_rn(red[1][t], red[1][t + 64]);
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            r1 = __dadd_rn(r1, __shfl_down(r1, s, 64));
            r2 = __dadd_rn(r2, __shfl_down(r2, s, 64));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ the pass
// grid G <= RPNET_REGION_MAX_BLOCKS; block b takes the chunks b, b + G, ...; `image` may be null.  acc: int64 [L][20], cleared.
template <class T, class I>
__global__ __launch_bounds__(256) void region_pass_kernel(const T* __restrict__ labels, const I* __restrict__ image, const int lo, const int L,
                                                          const FastDiv dW, const FastDiv dH, const unsigned n, const unsigned n_chunks,
                                                          const int iters, reg_u64* __restrict__ n_outside, reg_u64* __restrict__ acc,
                                                          double* __restrict__ partials) {
    __shared__ unsigned pres[RPNET_REGION_MAX_LABELS / 32];
    __shared__ double red[2][256];
    __shared__ double P[RPNET_REGION_MAX_LABELS][2];
    __shared__ unsigned wv[4][kRegCols];
    __shared__ unsigned out_sum;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned W = dW.d, H = dH.d;
    P[t][0] = P[t][1] = 0.0;
    if (t == 0) out_sum = 0u;
    unsigned outside = 0u;
    for (int it = 0; it < iters; ++it) {
        const unsigned chunk = (unsigned)it * gridDim.x + blockIdx.x;
        if (chunk >= n_chunks) break;                   // the same for every thread of the block
        if (t < RPNET_REGION_MAX_LABELS / 32) pres[t] = 0u;
        __syncthreads();
        const unsigned base = chunk * (unsigned)RPNET_REGION_CHUNK + (unsigned)(kRegLane * t);
        const int cnt = base < n ? (int)min((unsigned)kRegLane, n - base) : 0;
        int code[kRegLane];                             // the label where it is tallied, else -1
        {
            T lv[kRegLane];
            reg_load16(labels, base, cnt, lv);
#pragma unroll
            for (int j = 0; j < kRegLane; ++j) {
                const int l = j < cnt ? reg_label(lv[j], L) : 0;
                if (l < 0) ++outside;
                code[j] = (j < cnt && l >= lo) ? l : -1;
            }
        }
        float iv[kRegLane];
        if (image) {
            I raw[kRegLane];
            reg_load16(image, base, cnt, raw);
#pragma unroll
            for (int j = 0; j < kRegLane; ++j) iv[j] = (float)raw[j];
        } else {
#pragma unroll
            for (int j = 0; j < kRegLane; ++j) iv[j] = 0.0f;
        }
        const int first = __builtin_amdgcn_readfirstlane(code[0]);
        bool one = true;
#pragma unroll
        for (int j = 0; j < kRegLane; ++j) one = one && code[j] == first;
        if (__all(one)) {                               // the whole wave holds one label, or nothing that is tallied
            if (lane == 0 && first >= 0) atomicOr(&pres[first >> 5], 1u << (first & 31));
        } else {
#pragma unroll
            for (int j = 0; j < kRegLane; ++j)
                if (code[j] >= 0 && (j == 0 || code[j] != code[j - 1])) atomicOr(&pres[code[j] >> 5], 1u << (code[j] & 31));
        }
        __syncthreads();
        unsigned q, z0;
        const unsigned x0 = dW.divmod(base, q);
        const unsigned y0 = dH.divmod(q, z0);
        for (int w = 0; w < RPNET_REGION_MAX_LABELS / 32; ++w) {
            unsigned m = pres[w];                       // the same for every thread
            for (int k = __popc(m); k > 0; --k) {
                const int l = 32 * w + __ffs((int)m) - 1;
                m &= m - 1u;
                // the lane's share.  Sums of 16 voxels with coordinates below 1024 fit 32 bits; the extrema are maxima of the
                // encodings of the header, of which 0 says "none"
                unsigned c[kRegCols];
#pragma unroll
                for (int i = 0; i < kRegCols; ++i) c[i] = 0u;
                double a1 = 0.0, a2 = 0.0;
                unsigned z = z0, y = y0, x = x0;
#pragma unroll
                for (int j = 0; j < kRegLane; ++j) {
                    if (code[j] == l) {
                        c[0] += 1u;
                        c[1] = max(c[1], (unsigned)RPNET_CC_MAX_DIM - z);
                        c[2] = max(c[2], (unsigned)RPNET_CC_MAX_DIM - y);
                        c[3] = max(c[3], (unsigned)RPNET_CC_MAX_DIM - x);
                        c[4] = max(c[4], z + 1u);
                        c[5] = max(c[5], y + 1u);
                        c[6] = max(c[6], x + 1u);
                        c[7] += z;
                        c[8] += y;
                        c[9] += x;
                        c[10] += z * z;
                        c[11] += y * y;
                        c[12] += x * x;
                        c[13] += z * y;
                        c[14] += z * x;
                        c[15] += y * x;
                        const float v = iv[j];
                        if (image && (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u) {
                            const unsigned key = reg_key(v);
                            c[16] += 1u;
                            c[17] = max(c[17], 0xFFFFFFFFu - key);
                            c[18] = max(c[18], key);
                            const double dv = (double)v;
                            a1 = __dadd_rn(a1, dv);
                            a2 = __dadd_rn(a2, __dmul_rn(dv, dv));
                        }
                    }
                    if (++x == W) {
                        x = 0u;
                        if (++y == H) {
                            y = 0u;
                            ++z;
                        }
                    }
                }
                red[0][t] = a1;
                red[1][t] = a2;
                if (__any(c[0] != 0u)) {                // the same for every lane of the wave
#pragma unroll
                    for (int i = 0; i < kRegCols - 1; ++i) {
                        const bool is_max = (i >= 1 && i <= 6) || i == 17 || i == 18;
                        c[i] = is_max ? reg_wave_max(c[i]) : reg_wave_add(c[i]);
                    }
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < kRegCols; ++i) wv[wave][i] = c[i];
                    }
                } else if (lane < kRegCols) {
                    wv[wave][lane] = 0u;
                }
                __syncthreads();
                double r1 = 0.0, r2 = 0.0;
                reg_tree(red, t, r1, r2);
                if (t == 0) {
                    P[l][0] = __dadd_rn(P[l][0], r1);
                    P[l][1] = __dadd_rn(P[l][1], r2);
                }
                if (wave == 1 && lane < kRegCols - 1) {         // the four waves' shares of one column, into the accumulators
                    const int i = lane;
                    const bool is_max = (i >= 1 && i <= 6) || i == 17 || i == 18;
                    const unsigned s0 = wv[0][i], s1 = wv[1][i], s2 = wv[2][i], s3 = wv[3][i];
                    reg_u64* dst = acc + (size_t)l * kRegCols + i;
                    if (is_max) {
                        const unsigned v = max(max(s0, s1), max(s2, s3));
                        if (v) atomicMax(dst, (reg_u64)v);
                    } else {
                        const reg_u64 v = (reg_u64)s0 + s1 + s2 + s3;
                        if (v) atomicAdd(dst, v);
                    }
                }
                __syncthreads();                        // red and wv are free again
            }
        }
        __syncthreads();                                // every thread has read pres
    }
    outside = reg_wave_add(outside);
    if (lane == 0 && outside) atomicAdd(&out_sum, outside);
    __syncthreads();
    if (t == 0 && out_sum) atomicAdd(n_outside, (reg_u64)out_sum);
    if (image && t < L) {
        double* p = partials + ((size_t)blockIdx.x * L + t) * 2;
        p[0] = P[t][0];
        p[1] = P[t][1];
    }
}

// ------------------------------------------------------------------------------------------------------------------ the fold
// grid L, one block of 256 threads per label: the SUM of rpnet_fusion_abi.h over the G partials, and the row decoded from the accumulators
__global__ __launch_bounds__(256) void region_fold_kernel(const reg_u64* __restrict__ acc, const double* __restrict__ partials, const int G,
                                                          const int lo, const int L, const int D, const int H, const int W, const int has_image,
                                                          long long* __restrict__ rows_i, double* __restrict__ rows_f) {
    __shared__ double red[2][256];
    const int t = threadIdx.x, l = blockIdx.x;
    if (t < kRegCols) {
        const long long v = (long long)acc[(size_t)l * kRegCols + t];
        long long r = v;
        if (t >= 1 && t <= 3)
            r = v ? (long long)RPNET_CC_MAX_DIM - v : (long long)(t == 1 ? D : (t == 2 ? H : W));
        else if (t >= 4 && t <= 6)
            r = v - 1;
        else if (t == 17)
            r = 0xFFFFFFFFll - v;
        else if (t == 19)
            r = 0;
        rows_i[(size_t)l * kRegCols + t] = r;
    }
    if (!rows_f) return;                                // the same for every thread
    if (!has_image || l < lo) {
        if (t < RPNET_REGION_FROW) rows_f[(size_t)l * RPNET_REGION_FROW + t] = 0.0;
        return;
    }
    double a1 = 0.0, a2 = 0.0;
    for (int b = t; b < G; b += 256) {
        const double* p = partials + ((size_t)b * L + l) * 2;
        a1 = __dadd_rn(a1, p[0]);
        a2 = __dadd_rn(a2, p[1]);
    }
    red[0][t] = a1;
    red[1][t] = a2;
    __syncthreads();
    double r1 = 0.0, r2 = 0.0;
    reg_tree(red, t, r1, r2);
    if (t == 0) {
        rows_f[(size_t)l * RPNET_REGION_FROW + 0] = r1;
        rows_f[(size_t)l * RPNET_REGION_FROW + 1] = r2;
    }
}

const size_t kRegLabelElem[4] = {1, 4, 8, 4};
const size_t kRegImageElem[2] = {4, 2};

struct RegLaunch {
    const void *labels, *image;
    int lo, L;
    FastDiv dW, dH;
    unsigned n, n_chunks;
    int G, iters;
    reg_u64 *n_outside, *acc;
    double* partials;
};

template <class T, class I>
static void reg_launch_pass(const RegLaunch& a, hipStream_t st) {
    hipLaunchKernelGGL((region_pass_kernel<T, I>), dim3(a.G), dim3(256), 0, st, static_cast<const T*>(a.labels), static_cast<const I*>(a.image),
                       a.lo, a.L, a.dW, a.dH, a.n, a.n_chunks, a.iters, a.n_outside, a.acc, a.partials);
}
template <class T>
static void reg_launch_image(const RegLaunch& a, int image_kind, hipStream_t st) {
    if (a.image && image_kind == RPNET_PREP_I16)
        reg_launch_pass<T, int16_t>(a, st);
    else
        reg_launch_pass<T, float>(a, st);
}

}  // namespace
}  // namespace rpnet

extern "C" int rpnet_region_abi_version(void) { return RPNET_REGION_ABI_VERSION; }

extern "C" size_t rpnet_region_workspace_bytes(int D, int H, int W, int L) {
    using namespace rpnet;
    if (!reg_dims_ok(D, H, W) || L < 1 || L > RPNET_REGION_MAX_LABELS) {
        set_error("region_workspace_bytes: D=%d H=%d W=%d L=%d (every extent 1..%d, L 1..%d)", D, H, W, L, RPNET_CC_MAX_DIM, RPNET_REGION_MAX_LABELS);
        return 0;
    }
    return reg_need(D, H, W, L);
}

extern "C" int rpnet_region_stats(const void* labels, int label_kind, const void* image, int image_kind, int D, int H, int W, int lo, int L,
                                  int64_t* rows_i, double* rows_f, int64_t row, int64_t n_rows, void* workspace, size_t workspace_bytes,
                                  rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "region_stats";
    RPNET_REQUIRE(labels && rows_i && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(!image || rows_f, RPNET_ERR_ARG, "%s: an image needs rows_f", fn);
    RPNET_REQUIRE(label_kind >= RPNET_CC_U8 && label_kind <= RPNET_CC_F32, RPNET_ERR_ARG,
                  "%s: label kind %d (0 uint8, 1 int32, 2 int64, 3 float32)", fn, label_kind);
    RPNET_REQUIRE(!image || image_kind == RPNET_PREP_F32 || image_kind == RPNET_PREP_I16, RPNET_ERR_ARG, "%s: image kind %d (0 float32, 1 int16)", fn,
                  image_kind);
    RPNET_REQUIRE(L >= 1 && L <= RPNET_REGION_MAX_LABELS, RPNET_ERR_ARG, "%s: L=%d (1..%d labels)", fn, L, RPNET_REGION_MAX_LABELS);
    RPNET_REQUIRE((lo == 0 || lo == 1) && (lo < L || (L == 1 && lo == 1)), RPNET_ERR_ARG, "%s: lo=%d with L=%d (lo is 0 or 1 and below L, or L = lo = 1)",
                  fn, lo, L);
    RPNET_REQUIRE(reg_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(n_rows >= 1 && row >= 0 && row < n_rows, RPNET_ERR_ARG, "%s: row %lld of tables of %lld rows", fn, (long long)row,
                  (long long)n_rows);
    const size_t need = reg_need(D, H, W, L);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)labels % kRegLabelElem[label_kind]) == 0 && (!image || ((uintptr_t)image % kRegImageElem[image_kind]) == 0) &&
                      ((uintptr_t)rows_i % 8) == 0 && ((uintptr_t)rows_f % 8) == 0 && ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: volumes must be aligned to their element, the tables to 8 and the workspace to 16 bytes", fn);

    char* ws = static_cast<char*>(workspace);
    RegLaunch a;
    a.labels = labels;
    a.image = image;
    a.lo = lo;
    a.L = L;
    a.dW = FastDiv((unsigned)W);
    a.dH = FastDiv((unsigned)H);
    a.n = (unsigned)((size_t)D * H * W);                // at most 2^30
    a.n_chunks = (unsigned)reg_chunks(D, H, W);
    a.G = (int)std::min<unsigned>(a.n_chunks, RPNET_REGION_MAX_BLOCKS);
    a.iters = (int)((a.n_chunks + (unsigned)a.G - 1) / (unsigned)a.G);
    a.n_outside = reinterpret_cast<reg_u64*>(ws + RPNET_REGION_OUTSIDE_OFFSET);
    a.acc = reinterpret_cast<reg_u64*>(ws + RPNET_REGION_HEAD_BYTES);
    a.partials = reinterpret_cast<double*>(ws + RPNET_REGION_HEAD_BYTES + (size_t)kRegAccBytes * L);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, RPNET_REGION_HEAD_BYTES + (size_t)kRegAccBytes * L, st) != hipSuccess) return check_launch(fn);
    switch (label_kind) {
        case RPNET_CC_U8: reg_launch_image<uint8_t>(a, image_kind, st); break;
        case RPNET_CC_I32: reg_launch_image<int32_t>(a, image_kind, st); break;
        case RPNET_CC_I64: reg_launch_image<int64_t>(a, image_kind, st); break;
        default: reg_launch_image<float>(a, image_kind, st);
    }
    hipLaunchKernelGGL(region_fold_kernel, dim3(L), dim3(256), 0, st, a.acc, a.partials, a.G, lo, L, D, H, W, image ? 1 : 0,
                       reinterpret_cast<long long*>(rows_i) + row * L * RPNET_REGION_IROW, rows_f ? rows_f + row * L * RPNET_REGION_FROW : nullptr);
    return check_launch(fn);
}
