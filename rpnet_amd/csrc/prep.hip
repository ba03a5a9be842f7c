// Body-mask preprocessing of a raw CT volume on the device (include/rpnet_prep_abi.h; rpnet_amd/preprocess.py): the per-slice threshold
// (fixed or Otsu), the connected region of a seed pixel per slice, and the pass that masks the volume and finds the bounding box of what
// is left.  Between them run rpnet_morph_apply (per slice) and rpnet_ccpost_fill_holes (slice mode), which this file does not touch.
//
// What was chosen.  All three walk the volume in lanes of 16 consecutive voxels: a lane loads its voxels with 16-byte loads and writes
// them with one 16-byte store wherever the address of its first voxel is 16-byte aligned (decided per lane, so an odd slice size only
// costs the lanes it misaligns), and touches no other element, so that an output may be its input.  The threshold and the select pass
// lay their lanes out per slice (grid.y = z) and never straddle two slices; the box pass lays them over the flat volume.
//   threshold   clear; min / max / finite count per slice through an order-preserving uint32 encoding (LDS per block, then one integer
//               atomic per block and word); the 128-bin histogram (LDS per block, then integer atomicAdd of the bins the block met);
//               the mask pass, in which every block redoes the scan of the definition from its slice's 128 counts (thread k forms
//               w(k), m(k) and val(k) in int64 / fp64, thread 0 walks the 127 values for the first maximum); the rows.
//   component   the phases of cc_phases.h as <false, true>: the object itself, no z link; then select and write against the root of
//               the slice's seed pixel, and the rows.  The instantiations of components.hip and cc_post.hip are theirs.
//   box         mask, write, and reduce the extents and counts in registers, LDS, then one integer atomic per block and word.
// The fp64 operations of the Otsu definition are spelled one rounding at a time and the file is built with -ffp-contract=off: a numpy
// restatement gets the same bins, the same k* and the same threshold bit for bit.
//
// Bounds: every loop runs to a count fixed when it is entered (the sweeps of a block, the 16 voxels of a lane, 128 bins), except the
// walks of cc_phases.h, which carry theirs and set the `overrun` word.  No thread waits on another block.
#include <climits>
#include <cmath>

#include "cc_phases.h"
#include "rpnet_prep_abi.h"

namespace rpnet {

constexpr int kPrepLane = 16;                       // voxels of a lane
constexpr int kPrepSliceBlocks = 64;                // blocks per slice at most (threshold, select)
constexpr int kPrepBins = RPNET_PREP_OTSU_BINS;
constexpr int kPrepCols = 136;                      // uint32 words of a slice in the threshold workspace: 544 bytes, a multiple of 16
constexpr int kPrepMin = 128, kPrepMax = 129, kPrepFg = 130, kPrepFinite = 131, kPrepK = 132;
constexpr int kPrepSeedCols = 4;                    // uint32 words of a slice in the component workspace: before, kept, components
static_assert(kPrepBins == 128 && kPrepCols * sizeof(unsigned) % 16 == 0, "one thread per bin, 16-byte rows");
static_assert((long long)RPNET_CC_MAX_DIM * RPNET_CC_MAX_DIM <= (1ll << 20), "a bin count fits uint32 and the Otsu numerator 2^53");

// An element kind: is it finite, its order-preserving uint32 code (a <= b  <=>  enc(a) <= enc(b); -0 is coded as +0), and back
template <class T>
struct PrepElem;
template <>
struct PrepElem<float> {
    static __device__ __forceinline__ bool finite(const float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
    static __device__ __forceinline__ unsigned enc(const float v) {
        const unsigned u = __float_as_uint(v + 0.0f);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    static __device__ __forceinline__ double dec(const unsigned e) { return (double)__uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }
};
template <>
struct PrepElem<int16_t> {
    static __device__ __forceinline__ bool finite(const int16_t) { return true; }
    static __device__ __forceinline__ unsigned enc(const int16_t v) { return (unsigned)((int)v + 32768); }
    static __device__ __forceinline__ double dec(const unsigned e) { return (double)((int)e - 32768); }
};

// the voxels of a lane: 16-byte accesses where the lane is whole and its first address aligned; v[j] = 0 beyond cnt
template <class T>
__device__ __forceinline__ void prep_load16(const T* p, const size_t base, const int cnt, T (&v)[kPrepLane]) {
    const T* q = p + base;
    if (cnt == kPrepLane && ((uintptr_t)q & 15u) == 0) {
        uint4 w[sizeof(T)];                         // 16 elements are sizeof(T) words of 16 bytes
#pragma unroll
        for (int k = 0; k < (int)sizeof(T); ++k) w[k] = reinterpret_cast<const uint4*>(q)[k];
        __builtin_memcpy(v, w, sizeof(w));
    } else {
#pragma unroll
        for (int j = 0; j < kPrepLane; ++j) v[j] = j < cnt ? q[j] : (T)0;
    }
}
template <class T>
__device__ __forceinline__ void prep_store16(T* p, const size_t base, const int cnt, const T (&v)[kPrepLane]) {
    T* q = p + base;
    if (cnt == kPrepLane && ((uintptr_t)q & 15u) == 0) {
        uint4 w[sizeof(T)];
        __builtin_memcpy(w, v, sizeof(w));
#pragma unroll
        for (int k = 0; k < (int)sizeof(T); ++k) reinterpret_cast<uint4*>(q)[k] = w[k];
    } else {
#pragma unroll
        for (int j = 0; j < kPrepLane; ++j)
            if (j < cnt) q[j] = v[j];
    }
}

// the bin of step 5: lo and scale are the slice's
__device__ __forceinline__ int prep_bin(const double v, const double lo, const double scale) {
    return min(kPrepBins - 1, (int)__dmul_rn(__dsub_rn(v, lo), scale));          // 0 <= the product <= 128 and a bit
}

// ------------------------------------------------------------------------------------------------------------- threshold
// tab: [D][kPrepCols].  grid ceil(D * kPrepCols / 256)
__global__ __launch_bounds__(256) void prep_thr_clear_kernel(unsigned* __restrict__ head, unsigned* __restrict__ tab, const unsigned words) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < kCcHeadBytes / sizeof(unsigned)) head[threadIdx.x] = 0u;
    if (i < words) tab[i] = (i % (unsigned)kPrepCols) == (unsigned)kPrepMin ? 0xFFFFFFFFu : 0u;
}

// grid (blocks per slice, D); a block sweeps `iters` times over 256 lanes of its slice; n = H * W, lanes = ceil(n / 16)
template <class T>
__global__ __launch_bounds__(256) void prep_minmax_kernel(const T* __restrict__ img, const int n, const int lanes, const int iters,
                                                          unsigned* __restrict__ tab) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned s[3];
    const int t = threadIdx.x, z = blockIdx.y;
    if (t < 3) s[t] = t == 0 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    unsigned mn = 0xFFFFFFFFu, mx = 0u, nf = 0u;
    for (int it = 0; it < iters; ++it) {
        const int lane = (blockIdx.x * iters + it) * 256 + t;
        if (lane >= lanes) continue;
        const int cnt = min(kPrepLane, n - lane * kPrepLane);
        T v[kPrepLane];
        prep_load16(img, (size_t)z * n + (size_t)lane * kPrepLane, cnt, v);
#pragma unroll
        for (int j = 0; j < kPrepLane; ++j) {
            if (j >= cnt || !PrepElem<T>::finite(v[j])) continue;
            const unsigned e = PrepElem<T>::enc(v[j]);
            mn = min(mn, e);
            mx = max(mx, e);
            ++nf;
        }
    }
    if (nf) {
        atomicMin(&s[0], mn);
        atomicMax(&s[1], mx);
        atomicAdd(&s[2], nf);
    }
    __syncthreads();
    unsigned* row = tab + (size_t)z * kPrepCols;
    if (s[2]) {
        if (t == 0) atomicMin(row + kPrepMin, s[0]);
        if (t == 1) atomicMax(row + kPrepMax, s[1]);
        if (t == 2) atomicAdd(row + kPrepFinite, s[2]);
    }
}

template <class T>
__global__ __launch_bounds__(256) void prep_hist_kernel(const T* __restrict__ img, const int n, const int lanes, const int iters, unsigned* tab) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned h[kPrepBins];
    const int t = threadIdx.x, z = blockIdx.y;
    unsigned* row = tab + (size_t)z * kPrepCols;
    const double lo = PrepElem<T>::dec(row[kPrepMin]), hi = PrepElem<T>::dec(row[kPrepMax]);
    if (row[kPrepFinite] == 0u || !(hi > lo)) return;                 // the same for every thread of the block
    if (t < kPrepBins) h[t] = 0u;
    __syncthreads();
    const double scale = __ddiv_rn((double)kPrepBins, __dsub_rn(hi, lo));
    for (int it = 0; it < iters; ++it) {
        const int lane = (blockIdx.x * iters + it) * 256 + t;
        if (lane >= lanes) continue;
        const int cnt = min(kPrepLane, n - lane * kPrepLane);
        T v[kPrepLane];
        prep_load16(img, (size_t)z * n + (size_t)lane * kPrepLane, cnt, v);
#pragma unroll
        for (int j = 0; j < kPrepLane; ++j)
            if (j < cnt && PrepElem<T>::finite(v[j])) atomicAdd(&h[prep_bin((double)v[j], lo, scale)], 1u);
    }
    __syncthreads();
    if (t < kPrepBins && h[t]) atomicAdd(row + t, h[t]);
}

template <class T, bool kOtsu>
__global__ __launch_bounds__(256) void prep_mask_kernel(const T* __restrict__ img, uint8_t* __restrict__ mask, const int n, const int lanes,
                                                        const int iters, const double thr, unsigned* tab) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned h[kPrepBins];
    __shared__ double sval[kPrepBins];
    __shared__ int sk;
    __shared__ unsigned sfg;
    const int t = threadIdx.x, z = blockIdx.y;
    unsigned* row = tab + (size_t)z * kPrepCols;
    double lo = 0.0, scale = 0.0;
    bool valid = !kOtsu;
    if (t == 0) {
        sk = -1;
        sfg = 0u;
    }
    if (kOtsu) {
        lo = PrepElem<T>::dec(row[kPrepMin]);
        const double hi = PrepElem<T>::dec(row[kPrepMax]);
        valid = row[kPrepFinite] != 0u && hi > lo;                      // the same for every thread of the block
        if (valid) {
            scale = __ddiv_rn((double)kPrepBins, __dsub_rn(hi, lo));
            if (t < kPrepBins) h[t] = row[t];
            __syncthreads();
            if (t < kPrepBins) {
                long long w = 0, m = 0, N = 0, M = 0;                   // w(t), m(t), N, m(127)
                for (int b = 0; b < kPrepBins; ++b) {
                    const long long c = (long long)h[b];
                    N += c;
                    M += b * c;
                    if (b <= t) {
                        w += c;
                        m += b * c;
                    }
                }
                double val = -1.0;                                      // below every val(k), which is >= 0
                if (t < kPrepBins - 1 && w > 0 && w < N) {
                    const double num = (double)(M * w - m * N);
                    val = __ddiv_rn(__dmul_rn(num, num), __dmul_rn((double)w, (double)(N - w)));
                }
                sval[t] = val;
            }
            __syncthreads();
            if (t == 0) {
                double best = -1.0;
                int k = -1;
                for (int b = 0; b < kPrepBins - 1; ++b)
                    if (sval[b] > best) {
                        best = sval[b];
                        k = b;
                    }
                sk = k;
            }
        }
    }
    __syncthreads();
    const int ks = sk;
    unsigned fg = 0u;
    for (int it = 0; it < iters; ++it) {
        const int lane = (blockIdx.x * iters + it) * 256 + t;
        if (lane >= lanes) continue;
        const int cnt = min(kPrepLane, n - lane * kPrepLane);
        const size_t base = (size_t)z * n + (size_t)lane * kPrepLane;
        T v[kPrepLane];
        uint8_t o[kPrepLane];
        prep_load16(img, base, cnt, v);
#pragma unroll
        for (int j = 0; j < kPrepLane; ++j) {
            bool f = false;
            if (j < cnt && valid) {
                if (kOtsu) f = PrepElem<T>::finite(v[j]) && prep_bin((double)v[j], lo, scale) > ks;
                else f = (double)v[j] > thr;                            // false for NaN
            }
            o[j] = (uint8_t)f;
            fg += f;
        }
        prep_store16(mask, base, cnt, o);
    }
    if (fg) atomicAdd(&sfg, fg);
    __syncthreads();
    if (t == 0) {
        if (sfg) atomicAdd(row + kPrepFg, sfg);
        if (blockIdx.x == 0) row[kPrepK] = (unsigned)ks;
    }
}

// one thread per slice
template <class T>
__global__ __launch_bounds__(64) void prep_thr_rows_kernel(const unsigned* __restrict__ tab, const int D, const int otsu, const double thr,
                                                           long long* __restrict__ rows_i, double* __restrict__ rows_f) {
    const int z = blockIdx.x * 64 + threadIdx.x;
    if (z >= D) return;
    const unsigned* row = tab + (size_t)z * kPrepCols;
    const unsigned nf = row[kPrepFinite];
    const double lo = nf ? PrepElem<T>::dec(row[kPrepMin]) : 0.0, hi = nf ? PrepElem<T>::dec(row[kPrepMax]) : 0.0;
    const int k = otsu ? (int)row[kPrepK] : -1;
    const double step = __ddiv_rn(__dsub_rn(hi, lo), (double)kPrepBins);
    rows_i[z * RPNET_PREP_THRESHOLD_ROW + 0] = (long long)nf;
    rows_i[z * RPNET_PREP_THRESHOLD_ROW + 1] = (long long)k;
    rows_i[z * RPNET_PREP_THRESHOLD_ROW + 2] = (long long)row[kPrepFg];
    rows_i[z * RPNET_PREP_THRESHOLD_ROW + 3] = 0ll;
    rows_f[z * RPNET_PREP_THRESHOLD_FROW + 0] = lo;
    rows_f[z * RPNET_PREP_THRESHOLD_FROW + 1] = hi;
    rows_f[z * RPNET_PREP_THRESHOLD_FROW + 2] = otsu ? __dadd_rn(lo, __dmul_rn((double)(k + 1), step)) : thr;
}

// ------------------------------------------------------------------------------------------------------- seeded component
// the head, then the 16-byte words of the size volume and of the per-slice counts behind it
__global__ __launch_bounds__(256) void prep_seed_clear_kernel(uint4* __restrict__ head, uint4* __restrict__ tail, const size_t n16, const int iters) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x < kCcHeadBytes / sizeof(uint4)) head[threadIdx.x] = zero;
    for (int it = 0; it < iters; ++it) {
        const size_t i = ((size_t)blockIdx.x * iters + it) * 256u + threadIdx.x;
        if (i < n16) tail[i] = zero;
    }
}

// grid (blocks per slice, D).  After the flatten launch parent[i] is the root of i (-1: not the object), so the pass holds no walk.
// `in` and `out` may be one volume: a lane reads its 16 voxels, then writes them.
__global__ __launch_bounds__(256) void prep_select_kernel(const uint8_t* in, uint8_t* out, const int cls, const int32_t* __restrict__ parent,
                                                          const int n, const int lanes, const int iters, const int seed, unsigned* __restrict__ cnts) {
    RPNET_PASS_PRIORITY();
    __shared__ unsigned sc[3];                      // before, kept, components
    const int t = threadIdx.x, z = blockIdx.y;
    if (t < 3) sc[t] = 0u;
    __syncthreads();
    const size_t slice = (size_t)z * n;
    const int root = parent[slice + seed];          // seed < n
    unsigned before = 0u, kept = 0u, ncomp = 0u;
    for (int it = 0; it < iters; ++it) {
        const int lane = (blockIdx.x * iters + it) * 256 + t;
        if (lane >= lanes) continue;
        const int cnt = min(kPrepLane, n - lane * kPrepLane);
        const size_t base = slice + (size_t)lane * kPrepLane;
        uint8_t v[kPrepLane], o[kPrepLane];
        int32_t p[kPrepLane];
        prep_load16(in, base, cnt, v);
        prep_load16(parent, base, cnt, p);
#pragma unroll
        for (int j = 0; j < kPrepLane; ++j) {
            const bool obj = j < cnt && p[j] >= 0, keep = obj && p[j] == root;
            before += obj;
            kept += keep;
            ncomp += obj && p[j] == (int)(base + j);                   // the root speaks for its component
            o[j] = obj ? (keep ? (uint8_t)cls : (uint8_t)0) : v[j];
        }
        prep_store16(out, base, cnt, o);
    }
    if (before) atomicAdd(&sc[0], before);
    if (kept) atomicAdd(&sc[1], kept);
    if (ncomp) atomicAdd(&sc[2], ncomp);
    __syncthreads();
    if (t < 3 && sc[t]) atomicAdd(cnts + (size_t)z * kPrepSeedCols + t, sc[t]);
}

__global__ __launch_bounds__(64) void prep_seed_rows_kernel(const int32_t* __restrict__ parent, const unsigned* __restrict__ cnts,
                                                            const CcHead* __restrict__ head, const int D, const int n, const int seed,
                                                            long long* __restrict__ stats) {
    const int z = blockIdx.x * 64 + threadIdx.x;
    if (z >= D) return;
    const unsigned* c = cnts + (size_t)z * kPrepSeedCols;
    stats[z * RPNET_PREP_SEED_ROW + 0] = parent[(size_t)z * n + seed] >= 0 ? 1ll : 0ll;
    stats[z * RPNET_PREP_SEED_ROW + 1] = (long long)c[0];
    stats[z * RPNET_PREP_SEED_ROW + 2] = (long long)c[1];
    stats[z * RPNET_PREP_SEED_ROW + 3] = head->overrun ? -1ll : (long long)c[2];
}

// ------------------------------------------------------------------------------------------------------------ mask and box
struct PrepBoxHead {                                // the 64 bytes of the box workspace
    int mn[3], mx[3];                               // z, y, x of the kept voxels
    unsigned overrun, pad;                          // RPNET_CC_OVERRUN_OFFSET: never set, the pass holds no walk
    unsigned long long n_kept, n_mask, spare[2];
};
static_assert(sizeof(PrepBoxHead) == kCcHeadBytes && offsetof(PrepBoxHead, overrun) == RPNET_CC_OVERRUN_OFFSET, "head layout");

__global__ __launch_bounds__(64) void prep_box_clear_kernel(PrepBoxHead* __restrict__ head) {
    const int t = threadIdx.x;
    if (t < 3) {
        head->mn[t] = INT_MAX;
        head->mx[t] = -1;
    }
    if (t == 3) head->overrun = head->pad = 0u;
    if (t == 4) head->n_kept = head->n_mask = 0ull;
    if (t == 5) head->spare[0] = head->spare[1] = 0ull;
}

// lanes over the flat volume; `img` and `out` may be one volume
template <class T>
__global__ __launch_bounds__(256) void prep_box_kernel(const T* img, const uint8_t* __restrict__ mask, T* out, const T fill, const double fill_d,
                                                       const int D, const int H, const int W, const FastDiv div_w, const FastDiv div_h, const size_t n,
                                                       const size_t n_lanes, const int iters, PrepBoxHead* __restrict__ head) {
    RPNET_PASS_PRIORITY();
    __shared__ int smn[3], smx[3];
    __shared__ unsigned sn[2];
    const int t = threadIdx.x;
    if (t < 3) {
        smn[t] = INT_MAX;
        smx[t] = -1;
    }
    if (t < 2) sn[t] = 0u;
    __syncthreads();
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {-1, -1, -1};
    unsigned nk = 0u, nm = 0u;
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)blockIdx.x * iters + it) * 256u + t;
        if (lane >= n_lanes) continue;
        const size_t base = lane * kPrepLane;
        const int cnt = (int)std::min<size_t>((size_t)kPrepLane, n - base);
        T v[kPrepLane], o[kPrepLane];
        uint8_t m[kPrepLane];
        prep_load16(img, base, cnt, v);
        prep_load16(mask, base, cnt, m);
        unsigned q, zz;
        int x = (int)div_w.divmod((unsigned)base, q);                  // base < 2^30
        int y = (int)div_h.divmod(q, zz), z = (int)zz;
#pragma unroll
        for (int j = 0; j < kPrepLane; ++j) {
            const bool in_mask = j < cnt && m[j] != 0, keep = in_mask && (double)v[j] > fill_d;
            o[j] = in_mask ? v[j] : fill;
            nm += in_mask;
            if (keep) {
                ++nk;
                mn[0] = min(mn[0], z), mx[0] = max(mx[0], z);
                mn[1] = min(mn[1], y), mx[1] = max(mx[1], y);
                mn[2] = min(mn[2], x), mx[2] = max(mx[2], x);
            }
            if (++x == W) {
                x = 0;
                if (++y == H) y = 0, ++z;
            }
        }
        prep_store16(out, base, cnt, o);
    }
    if (nk) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&smn[a], mn[a]);
            atomicMax(&smx[a], mx[a]);
        }
        atomicAdd(&sn[0], nk);
    }
    if (nm) atomicAdd(&sn[1], nm);
    __syncthreads();
    if (sn[0]) {
        if (t < 3) atomicMin(&head->mn[t], smn[t]);
        if (t >= 3 && t < 6) atomicMax(&head->mx[t - 3], smx[t - 3]);
        if (t == 6) atomicAdd(&head->n_kept, (unsigned long long)sn[0]);
    }
    if (t == 7 && sn[1]) atomicAdd(&head->n_mask, (unsigned long long)sn[1]);
}

__global__ __launch_bounds__(64) void prep_box_row_kernel(const PrepBoxHead* __restrict__ head, long long* __restrict__ row) {
    const int t = threadIdx.x;
    const bool any = head->n_kept != 0ull;
    if (t < 3) {
        row[2 * t] = any ? (long long)head->mn[t] : -1ll;
        row[2 * t + 1] = any ? (long long)head->mx[t] : -1ll;
    }
    if (t == 3) row[6] = (long long)head->n_kept;
    if (t == 4) row[7] = (long long)head->n_mask;
}

// ------------------------------------------------------------------------------------------------------------------- host
static inline bool prep_kind_ok(int kind) { return kind == RPNET_PREP_F32 || kind == RPNET_PREP_I16; }
static inline size_t prep_elem(int kind) { return kind == RPNET_PREP_F32 ? 4 : 2; }
static inline size_t prep_thr_need(int D) { return kCcHeadBytes + (size_t)D * kPrepCols * sizeof(unsigned); }
static inline size_t prep_seed_need(int D, int H, int W) { return kCcHeadBytes + 2 * cc_vol_bytes(D, H, W) + (size_t)D * kPrepSeedCols * sizeof(unsigned); }
static inline bool prep_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}
// blocks per slice and sweeps per block of a per-slice launch over `lanes` lanes
static inline int prep_slice_blocks(int lanes) { return std::min(cdiv(lanes, 256), kPrepSliceBlocks); }
static inline int prep_slice_iters(int lanes, int blocks) { return cdiv(lanes, (long)blocks * 256); }

template <class T>
static void prep_threshold_run(const void* img, uint8_t* mask, int D, int H, int W, bool otsu, double t, int64_t* rows_i, double* rows_f, void* ws,
                               hipStream_t st) {
    const T* p = static_cast<const T*>(img);
    unsigned* head = static_cast<unsigned*>(ws);
    unsigned* tab = head + kCcHeadBytes / sizeof(unsigned);
    const int n = H * W, lanes = cdiv(n, kPrepLane), blocks = prep_slice_blocks(lanes), iters = prep_slice_iters(lanes, blocks);
    const unsigned words = (unsigned)D * kPrepCols;
    const dim3 grid(blocks, D);
    hipLaunchKernelGGL(prep_thr_clear_kernel, dim3(cdiv(words, 256)), dim3(256), 0, st, head, tab, words);
    hipLaunchKernelGGL(prep_minmax_kernel<T>, grid, dim3(256), 0, st, p, n, lanes, iters, tab);
    if (otsu) {
        hipLaunchKernelGGL(prep_hist_kernel<T>, grid, dim3(256), 0, st, p, n, lanes, iters, tab);
        hipLaunchKernelGGL((prep_mask_kernel<T, true>), grid, dim3(256), 0, st, p, mask, n, lanes, iters, t, tab);
    } else {
        hipLaunchKernelGGL((prep_mask_kernel<T, false>), grid, dim3(256), 0, st, p, mask, n, lanes, iters, t, tab);
    }
    hipLaunchKernelGGL(prep_thr_rows_kernel<T>, dim3(cdiv(D, 64)), dim3(64), 0, st, tab, D, otsu ? 1 : 0, t, reinterpret_cast<long long*>(rows_i), rows_f);
}

template <class T>
static void prep_box_run(const void* img, const uint8_t* mask, void* out, double fill, int D, int H, int W, int64_t* row, void* ws, hipStream_t st) {
    const size_t n = (size_t)D * H * W, n_lanes = (n + kPrepLane - 1) / kPrepLane;
    const int blocks = cc_sweep_blocks(n_lanes), iters = cc_sweep_iters(n_lanes, blocks);
    PrepBoxHead* head = static_cast<PrepBoxHead*>(ws);
    hipLaunchKernelGGL(prep_box_clear_kernel, dim3(1), dim3(64), 0, st, head);
    hipLaunchKernelGGL(prep_box_kernel<T>, dim3(blocks), dim3(256), 0, st, static_cast<const T*>(img), mask, static_cast<T*>(out), (T)fill, fill, D, H, W,
                       FastDiv((unsigned)W), FastDiv((unsigned)H), n, n_lanes, iters, head);
    hipLaunchKernelGGL(prep_box_row_kernel, dim3(1), dim3(64), 0, st, head, reinterpret_cast<long long*>(row));
}

}  // namespace rpnet

extern "C" int rpnet_prep_abi_version(void) { return RPNET_PREP_ABI_VERSION; }

#define RPNET_PREP_QUERY(name, words, bytes)                                                                      \
    extern "C" size_t name(int D, int H, int W) {                                                                 \
        using namespace rpnet;                                                                                    \
        if (!cc_dims_ok(D, H, W)) {                                                                               \
            set_error(words ": D=%d H=%d W=%d (every extent 1..%d)", D, H, W, RPNET_CC_MAX_DIM);                  \
            return 0;                                                                                             \
        }                                                                                                         \
        return (bytes);                                                                                           \
    }
RPNET_PREP_QUERY(rpnet_prep_threshold_workspace_bytes, "prep_threshold", prep_thr_need(D))
RPNET_PREP_QUERY(rpnet_prep_seeded_component_workspace_bytes, "prep_seeded_component", prep_seed_need(D, H, W))
RPNET_PREP_QUERY(rpnet_prep_mask_bbox_workspace_bytes, "prep_mask_bbox", kCcHeadBytes)
#undef RPNET_PREP_QUERY

extern "C" int rpnet_prep_threshold(const void* img, int kind, uint8_t* mask, int D, int H, int W, int mode, double t, int64_t* rows_i, double* rows_f,
                                    void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "prep_threshold";
    RPNET_REQUIRE(img && mask && rows_i && rows_f && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(prep_kind_ok(kind), RPNET_ERR_ARG, "%s: element kind %d (0 float32, 1 int16)", fn, kind);
    RPNET_REQUIRE(mode == RPNET_PREP_FIXED || mode == RPNET_PREP_OTSU, RPNET_ERR_ARG, "%s: mode %d (0 fixed, 1 Otsu)", fn, mode);
    RPNET_REQUIRE(mode == RPNET_PREP_OTSU || !std::isnan(t), RPNET_ERR_ARG, "%s: the threshold is NaN", fn);
    RPNET_REQUIRE(cc_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    const size_t need = prep_thr_need(D), n = (size_t)D * H * W;
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)img % prep_elem(kind)) == 0 && ((uintptr_t)rows_i % 8) == 0 && ((uintptr_t)rows_f % 8) == 0 &&
                      ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: the image must be aligned to its element, the tables to 8 and the workspace to 16 bytes", fn);
    RPNET_REQUIRE(prep_disjoint(img, n * prep_elem(kind), mask, n), RPNET_ERR_ARG, "%s: mask overlaps img", fn);
    if (kind == RPNET_PREP_F32)
        prep_threshold_run<float>(img, mask, D, H, W, mode == RPNET_PREP_OTSU, t, rows_i, rows_f, workspace, (hipStream_t)stream);
    else
        prep_threshold_run<int16_t>(img, mask, D, H, W, mode == RPNET_PREP_OTSU, t, rows_i, rows_f, workspace, (hipStream_t)stream);
    return check_launch(fn);
}

extern "C" int rpnet_prep_seeded_component(const uint8_t* in, uint8_t* out, int cls, int D, int H, int W, int seed_y, int seed_x, int connectivity,
                                           int64_t* stats, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "prep_seeded_component";
    RPNET_REQUIRE(in && out && stats && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(cls >= 1 && cls <= 255, RPNET_ERR_ARG, "%s: class %d (1..255: the volumes are uint8)", fn, cls);
    RPNET_REQUIRE(connectivity == 4 || connectivity == 8, RPNET_ERR_ARG, "%s: connectivity %d (4 or 8: every slice is its own image)", fn, connectivity);
    RPNET_REQUIRE(cc_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(seed_y >= 0 && seed_y < H && seed_x >= 0 && seed_x < W, RPNET_ERR_ARG, "%s: seed (y=%d, x=%d) outside the %d x %d slice", fn, seed_y,
                  seed_x, H, W);
    const size_t need = prep_seed_need(D, H, W), n = (size_t)D * H * W, vb = cc_vol_bytes(D, H, W);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)stats % 8) == 0 && ((uintptr_t)workspace % 16) == 0, RPNET_ERR_ARG,
                  "%s: the table must be aligned to 8 and the workspace to 16 bytes", fn);
    RPNET_REQUIRE(in == out || prep_disjoint(in, n, out, n), RPNET_ERR_ARG, "%s: out overlaps in (in place means out == in)", fn);
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    CcHead* head = reinterpret_cast<CcHead*>(ws);
    int32_t* parent = reinterpret_cast<int32_t*>(ws + kCcHeadBytes);
    int32_t* size = reinterpret_cast<int32_t*>(ws + kCcHeadBytes + vb);
    unsigned* cnts = reinterpret_cast<unsigned*>(ws + kCcHeadBytes + 2 * vb);
    const size_t n16 = vb / sizeof(uint4) + (size_t)D * kPrepSeedCols * sizeof(unsigned) / sizeof(uint4);
    const int cblocks = cc_sweep_blocks(n16);
    hipLaunchKernelGGL(prep_seed_clear_kernel, dim3(cblocks), dim3(256), 0, st, reinterpret_cast<uint4*>(head), reinterpret_cast<uint4*>(size), n16,
                       cc_sweep_iters(n16, cblocks));
    const dim3 tiles(cdiv(W, kCcTX), cdiv(H, kCcTY), cdiv(D, kCcTZ));
    const int blocks = cc_sweep_blocks(n), iters = cc_sweep_iters(n, blocks), conn8 = connectivity == 8;
    hipLaunchKernelGGL((cc_local_kernel<false, true>), tiles, dim3(256), 0, st, static_cast<const void*>(in), (int)RPNET_CC_U8, cls, D, H, W, conn8, parent,
                       head);
    hipLaunchKernelGGL(cc_merge_kernel<true>, dim3(blocks), dim3(256), 0, st, parent, D, H, W, conn8, FastDiv((unsigned)W), FastDiv((unsigned)H), n, iters,
                       head);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks), dim3(256), 0, st, parent, size, static_cast<int32_t*>(nullptr), n, iters, head);
    const int sn = H * W, lanes = cdiv(sn, kPrepLane), sblocks = prep_slice_blocks(lanes), siters = prep_slice_iters(lanes, sblocks);
    const int seed = seed_y * W + seed_x;
    hipLaunchKernelGGL(prep_select_kernel, dim3(sblocks, D), dim3(256), 0, st, in, out, cls, parent, sn, lanes, siters, seed, cnts);
    hipLaunchKernelGGL(prep_seed_rows_kernel, dim3(cdiv(D, 64)), dim3(64), 0, st, parent, cnts, head, D, sn, seed, reinterpret_cast<long long*>(stats));
    return check_launch(fn);
}

extern "C" int rpnet_prep_mask_bbox(const void* img, int kind, const uint8_t* mask, void* out, double fill, int D, int H, int W, int64_t* rows,
                                    int64_t row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "prep_mask_bbox";
    RPNET_REQUIRE(img && mask && out && rows && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(prep_kind_ok(kind), RPNET_ERR_ARG, "%s: element kind %d (0 float32, 1 int16)", fn, kind);
    const bool fill_ok = kind == RPNET_PREP_F32 ? (std::isfinite(fill) && (double)(float)fill == fill)
                                                : (fill >= -32768.0 && fill <= 32767.0 && std::floor(fill) == fill);
    RPNET_REQUIRE(fill_ok, RPNET_ERR_ARG, "%s: fill %g is not a value of element kind %d", fn, fill, kind);
    RPNET_REQUIRE(cc_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(n_rows >= 1 && row >= 0 && row < n_rows, RPNET_ERR_ARG, "%s: row %lld of a table of %lld rows", fn, (long long)row, (long long)n_rows);
    RPNET_REQUIRE(workspace_bytes >= kCcHeadBytes, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, kCcHeadBytes);
    const size_t es = prep_elem(kind), n = (size_t)D * H * W;
    RPNET_REQUIRE(((uintptr_t)img % es) == 0 && ((uintptr_t)out % es) == 0 && ((uintptr_t)rows % 8) == 0 && ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: the volumes must be aligned to their element, the table to 8 and the workspace to 16 bytes", fn);
    RPNET_REQUIRE((img == out || prep_disjoint(img, n * es, out, n * es)) && prep_disjoint(mask, n, out, n * es), RPNET_ERR_ARG,
                  "%s: out overlaps img or mask (in place means out == img)", fn);
    int64_t* r = rows + row * RPNET_PREP_BBOX_ROW;
    if (kind == RPNET_PREP_F32)
        prep_box_run<float>(img, mask, out, fill, D, H, W, r, workspace, (hipStream_t)stream);
    else
        prep_box_run<int16_t>(img, mask, out, fill, D, H, W, r, workspace, (hipStream_t)stream);
    return check_launch(fn);
}
