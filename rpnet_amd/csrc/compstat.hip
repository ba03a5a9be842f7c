// Per-component statistics of a segmented volume (include/rpnet_compstat_abi.h): the dense renumbering of the sparse labels of
// rpnet_cc_label by a fixed-order exclusive scan over the roots, and one pass that tallies, per component id, the geometry of
// rpnet_region_abi.h, exact integer sums of the quantised image and the overlap with a class of a second volume.
//
// The pass: a block of 256 lanes owns a chunk of 4096 voxels, 16 consecutive ones per lane.  The ids of a chunk are gathered in an LDS
// table of 128 slots (an id and 24 int64 accumulators, 25096 bytes of LDS per block).  The compiler gives the pass 104 to 112 VGPRs
// and no scratch: four waves per SIMD, four blocks per compute unit, 40 KiB of LDS each, of which 128 slots are the largest power of
// two that fits (the hash masks with the slot count).  A wave whose 1024 voxels hold one id
// folds them by wave reductions and adds once; elsewhere a lane folds its runs of equal ids in registers and adds once per run.  At
// the end of the chunk one thread per (slot, column) adds what is not the identity to the row by one global integer atomic.  A run
// that finds no slot within 8 probes adds to the row directly.  The extrema are maxima of encodings of which 0 is the identity, so
// one memset clears the rows, and a decode launch rewrites those columns in place.
//
// Bounds: every loop runs to a count fixed when it is entered (the trips of a block, the 16 voxels of a lane, the 8 probes, the tiles
// of the scan).  Atomics are integer ones only, so their order does not reach the result.  No block waits for another; what a launch
// gathers, an earlier launch wrote.  The gather of the renumbering checks the label against the volume and the root before it reads.
#include <algorithm>

#include "common.h"
#include "rpnet_compstat_abi.h"

namespace rpnet {
namespace {

typedef unsigned long long cs_u64;
constexpr int kCsLane = 16;                          // voxels of a lane
constexpr int kCsCols = RPNET_COMPSTAT_ROW;
constexpr int kCsSlots = RPNET_COMPSTAT_SLOTS;
constexpr int kCsProbes = 8;
constexpr unsigned kCsFirstBase = 1u << 30;          // column 23 holds 2^30 - index while it is accumulated

static inline bool cs_dims_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= RPNET_CC_MAX_DIM && H <= RPNET_CC_MAX_DIM && W <= RPNET_CC_MAX_DIM;
}
static inline size_t cs_chunks(int D, int H, int W) {
    return ((size_t)D * H * W + RPNET_COMPSTAT_CHUNK - 1) / RPNET_COMPSTAT_CHUNK;
}
static inline size_t cs_counts_bytes(int D, int H, int W) { return 4 * ((cs_chunks(D, H, W) + 3) / 4 * 4); }
static inline size_t cs_need(int D, int H, int W) {
    return RPNET_COMPSTAT_HEAD_BYTES + cs_counts_bytes(D, H, W) + 4 * (size_t)D * H * W;
}

__host__ __device__ constexpr bool cs_is_max(const int i) { return (i >= 1 && i <= 6) || i == 17 || i == 18 || i == 23; }

// the voxels of a lane: 16-byte accesses where the lane is whole and its first address aligned; v[j] = 0 beyond cnt
template <class T>
__device__ __forceinline__ void cs_load16(const T* p, const unsigned base, const int cnt, T (&v)[kCsLane]) {
    const T* q = p + base;
    if (cnt == kCsLane && ((uintptr_t)q & 15u) == 0) {
        constexpr int kWords = (int)sizeof(T);          // 16 elements are sizeof(T) words of 16 bytes
        uint4 w[kWords];
#pragma unroll
        for (int k = 0; k < kWords; ++k) w[k] = reinterpret_cast<const uint4*>(q)[k];
        __builtin_memcpy(v, w, sizeof(w));
    } else {
#pragma unroll
        for (int j = 0; j < kCsLane; ++j) v[j] = j < cnt ? q[j] : (T)0;
    }
}
__device__ __forceinline__ void cs_store16(int32_t* p, const unsigned base, const int cnt, const int32_t (&v)[kCsLane]) {
    int32_t* q = p + base;
    if (cnt == kCsLane && ((uintptr_t)q & 15u) == 0) {
        uint4 w[4];
        __builtin_memcpy(w, v, sizeof(w));
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<uint4*>(q)[k] = w[k];
    } else {
#pragma unroll
        for (int j = 0; j < kCsLane; ++j)
            if (j < cnt) q[j] = v[j];
    }
}

// the key of rpnet_volload_abi.h of a finite value
__device__ __forceinline__ unsigned cs_key(const float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned cs_wave_add(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned cs_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ cs_u64 cs_wave_add64(cs_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        v += ((cs_u64)hi << 32) | lo;
    }
    return v;
}

// exclusive prefix of v over the 256 threads of a block; total: the sum over the block, the same in every thread.  smem: 4 words;
// the caller's next use of smem is behind the barrier at the head of the next call
__device__ __forceinline__ unsigned cs_block_exclusive(const unsigned v, unsigned* smem, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) smem[wave] = inc;
    __syncthreads();
    const unsigned w0 = smem[0], w1 = smem[1], w2 = smem[2], w3 = smem[3];
    total = w0 + w1 + w2 + w3;
    const unsigned before = wave == 0 ? 0u : (wave == 1 ? w0 : (wave == 2 ? w0 + w1 : w0 + w1 + w2));
    return before + inc - v;
}

// ------------------------------------------------------------------------------------------------------------------ the renumbering
// the roots among the 16 voxels of a lane, as a bit mask
__device__ __forceinline__ unsigned cs_roots(const int32_t* __restrict__ labels, const unsigned base, const int cnt) {
    int32_t lv[kCsLane];
    cs_load16(labels, base, cnt, lv);
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < kCsLane; ++j)
        if (j < cnt && lv[j] == (int32_t)(base + (unsigned)j + 1u)) m |= 1u << j;
    return m;
}

// grid nc: counts[chunk] = the roots of the chunk
__global__ __launch_bounds__(256) void compstat_count_kernel(const int32_t* __restrict__ labels, const unsigned n, unsigned* __restrict__ counts) {
    __shared__ unsigned smem[4];
    const unsigned base = blockIdx.x * (unsigned)RPNET_COMPSTAT_CHUNK + (unsigned)(kCsLane * threadIdx.x);
    const int cnt = base < n ? (int)min((unsigned)kCsLane, n - base) : 0;
    const unsigned c = cs_wave_add((unsigned)__popc(cs_roots(labels, base, cnt)));
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = smem[0] + smem[1] + smem[2] + smem[3];
}

// ONE block: counts -> exclusive offsets in place, tile of 256 chunks by tile; head[0] = C
__global__ __launch_bounds__(RPNET_COMPSTAT_SCAN_THREADS) void compstat_scan_kernel(unsigned* __restrict__ counts, const unsigned nc, const int tiles,
                                                                                   cs_u64* __restrict__ head) {
    __shared__ unsigned smem[4];
    unsigned carry = 0u;
    for (int tile = 0; tile < tiles; ++tile) {
        const unsigned at = (unsigned)tile * RPNET_COMPSTAT_SCAN_THREADS + threadIdx.x;
        const unsigned v = at < nc ? counts[at] : 0u;
        unsigned total;
        const unsigned ex = cs_block_exclusive(v, smem, total);
        if (at < nc) counts[at] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) head[RPNET_COMPSTAT_COUNT_OFFSET / 8] = carry;
}

// grid nc: every root writes its id
__global__ __launch_bounds__(256) void compstat_roots_kernel(const int32_t* __restrict__ labels, const unsigned n, const unsigned* __restrict__ offsets,
                                                             int32_t* __restrict__ rank) {
    __shared__ unsigned smem[4];
    const unsigned base = blockIdx.x * (unsigned)RPNET_COMPSTAT_CHUNK + (unsigned)(kCsLane * threadIdx.x);
    const int cnt = base < n ? (int)min((unsigned)kCsLane, n - base) : 0;
    const unsigned m = cs_roots(labels, base, cnt);
    unsigned total;
    unsigned id = offsets[blockIdx.x] + cs_block_exclusive((unsigned)__popc(m), smem, total);
#pragma unroll
    for (int j = 0; j < kCsLane; ++j)
        if (m & (1u << j)) rank[base + (unsigned)j] = (int32_t)(++id);       // a set bit lies below cnt
}

// grid nc: dense[i] = rank[labels[i] - 1] where labels[i] names a root of the volume
__global__ __launch_bounds__(256) void compstat_gather_kernel(const int32_t* __restrict__ labels, const unsigned n, const int32_t* __restrict__ rank,
                                                              int32_t* __restrict__ dense, cs_u64* __restrict__ head) {
    __shared__ unsigned smem[4];
    const unsigned base = blockIdx.x * (unsigned)RPNET_COMPSTAT_CHUNK + (unsigned)(kCsLane * threadIdx.x);
    const int cnt = base < n ? (int)min((unsigned)kCsLane, n - base) : 0;
    int32_t lv[kCsLane], out[kCsLane];
    cs_load16(labels, base, cnt, lv);
    unsigned bad = 0u;
#pragma unroll
    for (int j = 0; j < kCsLane; ++j) {
        const int32_t l = lv[j];
        int32_t d = 0;
        if (j < cnt && l != 0) {
            const bool inside = l >= 1 && (unsigned)l <= n;
            if (inside && (j == 0 || l != lv[j - 1] || out[j - 1] == 0)) {
                if (labels[l - 1] == l) d = rank[l - 1];
            } else if (inside) {
                d = out[j - 1];                             // the same label as the voxel before, which named a root
            }
            if (d == 0) ++bad;
        }
        out[j] = d;
    }
    cs_store16(dense, base, cnt, out);
    bad = cs_wave_add(bad);
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned s = smem[0] + smem[1] + smem[2] + smem[3];
        if (s) atomicAdd(head + RPNET_COMPSTAT_INVALID_OFFSET / 8, (cs_u64)s);
    }
}

__global__ void compstat_stats_kernel(const cs_u64* __restrict__ head, long long* __restrict__ stats) {
    stats[0] = (long long)head[RPNET_COMPSTAT_COUNT_OFFSET / 8];
    stats[1] = (long long)head[RPNET_COMPSTAT_INVALID_OFFSET / 8];
    stats[2] = 0;
    stats[3] = 0;
}

// ------------------------------------------------------------------------------------------------------------------ the pass
// what a lane or a wave holds of one id: the 32-bit columns (16 voxels, or 1024 after the wave reductions, with coordinates below 1024
// stay below 2^31) and the three sums of the quantised values in 64 bits
struct CsRun {
    unsigned c[kCsCols];        // c[19..21] unused
    cs_u64 s1, s2lo, s2hi;
};

__device__ __forceinline__ void cs_clear(CsRun& r) {
#pragma unroll
    for (int i = 0; i < kCsCols; ++i) r.c[i] = 0u;
    r.s1 = r.s2lo = r.s2hi = 0ull;
}

__device__ __forceinline__ void cs_voxel(CsRun& r, const unsigned z, const unsigned y, const unsigned x, const unsigned index, const bool summed,
                                         const float v, const long long k, const bool overlap) {
    r.c[0] += 1u;
    r.c[1] = max(r.c[1], (unsigned)RPNET_CC_MAX_DIM - z);
    r.c[2] = max(r.c[2], (unsigned)RPNET_CC_MAX_DIM - y);
    r.c[3] = max(r.c[3], (unsigned)RPNET_CC_MAX_DIM - x);
    r.c[4] = max(r.c[4], z + 1u);
    r.c[5] = max(r.c[5], y + 1u);
    r.c[6] = max(r.c[6], x + 1u);
    r.c[7] += z;
    r.c[8] += y;
    r.c[9] += x;
    r.c[10] += z * z;
    r.c[11] += y * y;
    r.c[12] += x * x;
    r.c[13] += z * y;
    r.c[14] += z * x;
    r.c[15] += y * x;
    if (summed) {
        const unsigned key = cs_key(v);
        r.c[16] += 1u;
        r.c[17] = max(r.c[17], 0xFFFFFFFFu - key);
        r.c[18] = max(r.c[18], key);
        const cs_u64 kk = (cs_u64)(k * k);              // |k| < 2^31: below 2^62
        r.s1 += (cs_u64)k;                              // two's complement: the wrapped sum is the signed sum
        r.s2lo += kk & 0xFFFFFFFFull;
        r.s2hi += kk >> 32;
    }
    if (overlap) r.c[22] += 1u;
    r.c[23] = max(r.c[23], kCsFirstBase - index);
}

template <class P>
__device__ __forceinline__ void cs_add_run(P* dst, const CsRun& r) {
#pragma unroll
    for (int i = 0; i < kCsCols; ++i) {
        if (i >= 19 && i <= 21) continue;
        if (r.c[i]) {
            if (cs_is_max(i))
                atomicMax(dst + i, (cs_u64)r.c[i]);
            else
                atomicAdd(dst + i, (cs_u64)r.c[i]);
        }
    }
    if (r.s1) atomicAdd(dst + 19, r.s1);
    if (r.s2lo) atomicAdd(dst + 20, r.s2lo);
    if (r.s2hi) atomicAdd(dst + 21, r.s2hi);
}

// the run of `id` (1 .. max_components) into its slot, or into its row where no slot is found within the probes
__device__ __forceinline__ void cs_flush_run(const int id, const CsRun& r, int* slot_id, cs_u64 (*slot_acc)[kCsCols], cs_u64* __restrict__ rows) {
    const unsigned h = ((unsigned)id * 2654435761u) >> 25;             // 7 bits: kCsSlots = 128
    int slot = -1;
    for (int p = 0; p < kCsProbes; ++p) {
        const int s = (int)((h + (unsigned)p) & (unsigned)(kCsSlots - 1));
        const int seen = atomicCAS(&slot_id[s], 0, id);     // always the atomic: other lanes claim the same word
        if (seen == 0 || seen == id) {
            slot = s;
            break;
        }
    }
    if (slot >= 0)
        cs_add_run(&slot_acc[slot][0], r);
    else
        cs_add_run(rows + (size_t)(id - 1) * kCsCols, r);
}

__device__ __forceinline__ bool cs_is_class(const uint8_t v, const int cls) { return (int)v == cls; }
__device__ __forceinline__ bool cs_is_class(const int32_t v, const int cls) { return v == cls; }
__device__ __forceinline__ bool cs_is_class(const int64_t v, const int cls) { return v == (int64_t)cls; }
__device__ __forceinline__ bool cs_is_class(const float v, const int cls) { return v == (float)cls; }

// the voxels of a lane that hold other_cls in `other`, as a bit mask; the 16 elements are read like every other volume
template <class T>
__device__ __forceinline__ unsigned cs_overlap_mask(const T* __restrict__ other, const int other_cls, const unsigned base, const int cnt) {
    T ov[kCsLane];
    cs_load16(other, base, cnt, ov);
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < kCsLane; ++j)
        if (j < cnt && cs_is_class(ov[j], other_cls)) m |= 1u << j;
    return m;
}

// grid G <= RPNET_COMPSTAT_MAX_BLOCKS; block b takes the chunks b, b + G, ...; image and other may be null.  rows: the cleared row
// table int64 [max_components][24] of this call; head: C is read, n_beyond and the table's invalid word (cleared) are added to
template <class OT>
__global__ __launch_bounds__(256) void compstat_pass_kernel(const int32_t* __restrict__ dense, const void* __restrict__ image, const int image_kind,
                                                            const double scale, const OT* __restrict__ other, const int other_cls, const FastDiv dW, const FastDiv dH, const unsigned n,
                                                            const unsigned n_chunks, const int iters, const int max_components,
                                                            cs_u64* __restrict__ head, cs_u64* __restrict__ rows) {
    __shared__ cs_u64 slot_acc[kCsSlots][kCsCols];
    __shared__ int slot_id[kCsSlots];
    __shared__ unsigned tally[2];
    const int t = threadIdx.x, lane = t & 63;
    const unsigned W = dW.d, H = dH.d;
    const long long C = (long long)head[RPNET_COMPSTAT_COUNT_OFFSET / 8];      // written by an earlier launch
    for (int i = t; i < kCsSlots * kCsCols; i += 256) (&slot_acc[0][0])[i] = 0ull;
    if (t < kCsSlots) slot_id[t] = 0;
    if (t < 2) tally[t] = 0u;
    __syncthreads();
    unsigned beyond = 0u, invalid = 0u;
    for (int it = 0; it < iters; ++it) {
        const unsigned chunk = (unsigned)it * gridDim.x + blockIdx.x;
        if (chunk >= n_chunks) break;                   // the same for every thread of the block
        const unsigned base = chunk * (unsigned)RPNET_COMPSTAT_CHUNK + (unsigned)(kCsLane * t);
        const int cnt = base < n ? (int)min((unsigned)kCsLane, n - base) : 0;
        int code[kCsLane];                              // the id where the voxel is tallied, else 0
        {
            int32_t dv[kCsLane];
            cs_load16(dense, base, cnt, dv);
#pragma unroll
            for (int j = 0; j < kCsLane; ++j) {
                const int d = dv[j];                    // 0 beyond cnt
                int c = 0;
                if (d < 0 || (long long)d > C)
                    ++invalid;
                else if (d > max_components)
                    ++beyond;
                else
                    c = d;
                code[j] = c;
            }
        }
        const int first = __builtin_amdgcn_readfirstlane(code[0]);
        bool one = cnt == kCsLane;
        bool any = false;
#pragma unroll
        for (int j = 0; j < kCsLane; ++j) {
            one = one && code[j] == first;
            any = any || code[j] != 0;
        }
        const bool wave_one = __all(one) != 0;
        if (__any(any)) {                               // the same for every lane of the wave
            float iv[kCsLane];
            if (image && image_kind == RPNET_PREP_I16) {
                int16_t raw[kCsLane];
                cs_load16(static_cast<const int16_t*>(image), base, cnt, raw);
#pragma unroll
                for (int j = 0; j < kCsLane; ++j) iv[j] = (float)raw[j];
            } else if (image) {
                cs_load16(static_cast<const float*>(image), base, cnt, iv);
            } else {
#pragma unroll
                for (int j = 0; j < kCsLane; ++j) iv[j] = 0.0f;
            }
            const unsigned over = other ? cs_overlap_mask(other, other_cls, base, cnt) : 0u;
            unsigned q, z, y, x;
            x = dW.divmod(base, q);
            y = dH.divmod(q, z);
            CsRun r;
            cs_clear(r);
#pragma unroll
            for (int j = 0; j < kCsLane; ++j) {
                if (!wave_one && j > 0 && code[j] != code[j - 1] && code[j - 1] != 0) {
                    cs_flush_run(code[j - 1], r, slot_id, slot_acc, rows);
                    cs_clear(r);
                }
                if (code[j] != 0) {
                    const double k = rint((double)iv[j] * scale);       // the product is exact; a NaN or an infinity fails the comparison
                    const bool summed = image != nullptr && fabs(k) < 2147483648.0;
                    cs_voxel(r, z, y, x, base + (unsigned)j, summed, iv[j], summed ? (long long)k : 0ll, (over >> j) & 1u);
                }
                if (++x == W) {
                    x = 0u;
                    if (++y == H) {
                        y = 0u;
                        ++z;
                    }
                }
            }
            if (wave_one) {                             // first != 0 here: one id in the 1024 voxels of the wave
#pragma unroll
                for (int i = 0; i < kCsCols; ++i) {
                    if (i >= 19 && i <= 21) continue;
                    r.c[i] = cs_is_max(i) ? cs_wave_max(r.c[i]) : cs_wave_add(r.c[i]);
                }
                r.s1 = cs_wave_add64(r.s1);
                r.s2lo = cs_wave_add64(r.s2lo);
                r.s2hi = cs_wave_add64(r.s2hi);
                if (lane == 0) cs_flush_run(first, r, slot_id, slot_acc, rows);
            } else if (code[kCsLane - 1] != 0) {
                cs_flush_run(code[kCsLane - 1], r, slot_id, slot_acc, rows);
            }
        }
        __syncthreads();                                // every run of the chunk is in the table or in the rows
        for (int i = t; i < kCsSlots * kCsCols; i += 256) {
            const int s = i / kCsCols, col = i - s * kCsCols;
            const int id = slot_id[s];
            const cs_u64 v = slot_acc[s][col];
            if (id != 0 && v != 0ull) {
                cs_u64* dst = rows + (size_t)(id - 1) * kCsCols + col;
                if (cs_is_max(col))
                    atomicMax(dst, v);
                else
                    atomicAdd(dst, v);
                slot_acc[s][col] = 0ull;
            }
        }
        __syncthreads();                                // every thread has read the ids
        if (t < kCsSlots) slot_id[t] = 0;
        __syncthreads();
    }
    beyond = cs_wave_add(beyond);
    invalid = cs_wave_add(invalid);
    if (lane == 0) {
        if (beyond) atomicAdd(&tally[0], beyond);
        if (invalid) atomicAdd(&tally[1], invalid);
    }
    __syncthreads();
    if (t == 0) {
        if (tally[0]) atomicAdd(head + RPNET_COMPSTAT_BEYOND_OFFSET / 8, (cs_u64)tally[0]);
        if (tally[1]) atomicAdd(head + RPNET_COMPSTAT_TABLE_INVALID_OFFSET / 8, (cs_u64)tally[1]);
    }
}

// the encoded columns of every row, in place: one thread per entry
__global__ __launch_bounds__(256) void compstat_decode_kernel(long long* __restrict__ rows, const unsigned entries, const int D, const int H, const int W) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= entries) return;
    const unsigned col = i % (unsigned)kCsCols;
    if (!cs_is_max((int)col) || col == 18u) return;
    const long long v = rows[i];
    long long r;
    if (col >= 1u && col <= 3u)
        r = v ? (long long)RPNET_CC_MAX_DIM - v : (long long)(col == 1u ? D : (col == 2u ? H : W));
    else if (col >= 4u && col <= 6u)
        r = v - 1;
    else if (col == 17u)
        r = 0xFFFFFFFFll - v;
    else
        r = v ? (long long)kCsFirstBase - v : -1ll;
    rows[i] = r;
}

struct CsLaunch {
    const int32_t* dense;
    const void* image;
    int image_kind;
    double scale;
    const void* other;
    int other_cls;
    FastDiv dW, dH;
    unsigned n, n_chunks;
    int G, iters, max_components;
    cs_u64 *head, *rows;
};

template <class OT>
static void cs_launch_pass(const CsLaunch& a, hipStream_t st) {
    hipLaunchKernelGGL((compstat_pass_kernel<OT>), dim3(a.G), dim3(256), 0, st, a.dense, a.image, a.image_kind, a.scale, static_cast<const OT*>(a.other),
                       a.other_cls, a.dW, a.dH, a.n, a.n_chunks, a.iters, a.max_components, a.head, a.rows);
}

const size_t kCsOtherElem[4] = {1, 4, 8, 4};
const size_t kCsImageElem[2] = {4, 2};

}  // namespace
}  // namespace rpnet

extern "C" int rpnet_compstat_abi_version(void) { return RPNET_COMPSTAT_ABI_VERSION; }

extern "C" size_t rpnet_compstat_workspace_bytes(int D, int H, int W, int max_components) {
    using namespace rpnet;
    if (!cs_dims_ok(D, H, W) || max_components < 1 || max_components > RPNET_COMPSTAT_MAX_COMPONENTS) {
        set_error("compstat_workspace_bytes: D=%d H=%d W=%d max_components=%d (every extent 1..%d, max_components 1..%d)", D, H, W, max_components,
                  RPNET_CC_MAX_DIM, RPNET_COMPSTAT_MAX_COMPONENTS);
        return 0;
    }
    return cs_need(D, H, W);
}

extern "C" int rpnet_compstat_rank(const int32_t* labels, int D, int H, int W, int32_t* dense, int64_t* stats, int64_t stats_row, int64_t n_rows,
                                   void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "compstat_rank";
    RPNET_REQUIRE(labels && dense && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE((const void*)labels != (const void*)dense, RPNET_ERR_ARG, "%s: dense may not alias labels", fn);
    RPNET_REQUIRE(cs_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(!stats || (n_rows >= 1 && stats_row >= 0 && stats_row < n_rows), RPNET_ERR_ARG, "%s: row %lld of a table of %lld rows", fn,
                  (long long)stats_row, (long long)n_rows);
    const size_t need = cs_need(D, H, W);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)labels % 4) == 0 && ((uintptr_t)dense % 4) == 0 && ((uintptr_t)stats % 8) == 0 && ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: volumes must be aligned to 4, the table to 8 and the workspace to 16 bytes", fn);

    char* ws = static_cast<char*>(workspace);
    cs_u64* head = reinterpret_cast<cs_u64*>(ws);
    unsigned* counts = reinterpret_cast<unsigned*>(ws + RPNET_COMPSTAT_HEAD_BYTES);
    int32_t* rank = reinterpret_cast<int32_t*>(ws + RPNET_COMPSTAT_HEAD_BYTES + cs_counts_bytes(D, H, W));
    const unsigned n = (unsigned)((size_t)D * H * W);   // at most 2^30
    const unsigned nc = (unsigned)cs_chunks(D, H, W);   // at most 2^18
    const int tiles = (int)((nc + RPNET_COMPSTAT_SCAN_THREADS - 1) / RPNET_COMPSTAT_SCAN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, 16, st) != hipSuccess) return check_launch(fn);       // C and the rank's invalid word
    hipLaunchKernelGGL(compstat_count_kernel, dim3(nc), dim3(256), 0, st, labels, n, counts);
    hipLaunchKernelGGL(compstat_scan_kernel, dim3(1), dim3(RPNET_COMPSTAT_SCAN_THREADS), 0, st, counts, nc, tiles, head);
    hipLaunchKernelGGL(compstat_roots_kernel, dim3(nc), dim3(256), 0, st, labels, n, counts, rank);
    hipLaunchKernelGGL(compstat_gather_kernel, dim3(nc), dim3(256), 0, st, labels, n, rank, dense, head);
    if (stats)
        hipLaunchKernelGGL(compstat_stats_kernel, dim3(1), dim3(1), 0, st, head, reinterpret_cast<long long*>(stats) + stats_row * RPNET_COMPSTAT_STATS_ROW);
    return check_launch(fn);
}

extern "C" int rpnet_compstat_table(const int32_t* dense, const void* image, int image_kind, int scale_log2, const void* other, int other_kind,
                                    int other_cls, int D, int H, int W, int max_components, int64_t* rows, int64_t row, int64_t n_rows,
                                    void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "compstat_table";
    RPNET_REQUIRE(dense && rows && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(!image || image_kind == RPNET_PREP_F32 || image_kind == RPNET_PREP_I16, RPNET_ERR_ARG, "%s: image kind %d (0 float32, 1 int16)", fn,
                  image_kind);
    RPNET_REQUIRE(!image || (scale_log2 >= 0 && scale_log2 <= RPNET_COMPSTAT_MAX_SCALE_LOG2), RPNET_ERR_ARG, "%s: scale_log2=%d (0..%d)", fn, scale_log2,
                  RPNET_COMPSTAT_MAX_SCALE_LOG2);
    RPNET_REQUIRE(!other || (other_kind >= RPNET_CC_U8 && other_kind <= RPNET_CC_F32), RPNET_ERR_ARG,
                  "%s: other kind %d (0 uint8, 1 int32, 2 int64, 3 float32)", fn, other_kind);
    RPNET_REQUIRE(max_components >= 1 && max_components <= RPNET_COMPSTAT_MAX_COMPONENTS, RPNET_ERR_ARG, "%s: max_components=%d (1..%d)", fn,
                  max_components, RPNET_COMPSTAT_MAX_COMPONENTS);
    RPNET_REQUIRE(cs_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(n_rows >= 1 && row >= 0 && row < n_rows, RPNET_ERR_ARG, "%s: row %lld of a table of %lld rows", fn, (long long)row, (long long)n_rows);
    const size_t need = cs_need(D, H, W);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    RPNET_REQUIRE(((uintptr_t)dense % 4) == 0 && (!image || ((uintptr_t)image % kCsImageElem[image_kind]) == 0) &&
                      (!other || ((uintptr_t)other % kCsOtherElem[other_kind]) == 0) && ((uintptr_t)rows % 8) == 0 && ((uintptr_t)workspace % 16) == 0,
                  RPNET_ERR_ARG, "%s: volumes must be aligned to their element, the table to 8 and the workspace to 16 bytes", fn);

    char* ws = static_cast<char*>(workspace);
    cs_u64* head = reinterpret_cast<cs_u64*>(ws);
    const size_t row_entries = (size_t)max_components * RPNET_COMPSTAT_ROW;     // at most 2^16 * 24
    int64_t* mine = rows + row * (int64_t)row_entries;
    const unsigned n = (unsigned)((size_t)D * H * W);   // at most 2^30
    const unsigned nc = (unsigned)cs_chunks(D, H, W);
    const int G = (int)std::min<unsigned>(nc, RPNET_COMPSTAT_MAX_BLOCKS);
    const int iters = (int)((nc + (unsigned)G - 1) / (unsigned)G);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws + RPNET_COMPSTAT_BEYOND_OFFSET, 0, 16, st) != hipSuccess) return check_launch(fn);    // n_beyond and the table's invalid word
    if (hipMemsetAsync(mine, 0, 8 * row_entries, st) != hipSuccess) return check_launch(fn);
    CsLaunch a = {dense, image, image_kind, (double)(1u << (image ? scale_log2 : 0)), other, other_cls, FastDiv((unsigned)W), FastDiv((unsigned)H), n, nc,
                  G, iters, max_components, head, reinterpret_cast<cs_u64*>(mine)};
    switch (other ? other_kind : RPNET_CC_U8) {         // a null `other` reads nothing: any kind does
        case RPNET_CC_U8: cs_launch_pass<uint8_t>(a, st); break;
        case RPNET_CC_I32: cs_launch_pass<int32_t>(a, st); break;
        case RPNET_CC_I64: cs_launch_pass<int64_t>(a, st); break;
        default: cs_launch_pass<float>(a, st);
    }
    hipLaunchKernelGGL(compstat_decode_kernel, dim3((unsigned)((row_entries + 255) / 256)), dim3(256), 0, st, reinterpret_cast<long long*>(mine),
                       (unsigned)row_entries, D, H, W);
    return check_launch(fn);
}
