// Segmentation masks and Dice tallies of an evaluation call as ONE launch (rpnet_amd/volume.py).  The reference's driver
// (test_rpnet.py:189-246) takes softmax(dim=1)[:, 1] of the output and of every refinement iteration's logits, copies the
// probabilities to the host, thresholds at 0.5 there and counts |P and T|, |P|, |T| in numpy (utils/util.py:379-390): T + 1 softmax
// launches, T + 1 index launches and T + 1 blocking copies per model call.  Here a thread owns four neighbouring pixels of one image
// and walks the S sources (logit tensors [N][K][H][W], or 0/1 masks [N][H][W]: the driver's affine baseline) with 16-byte loads;
// every source value is read once, the labels once per thread.  Per source it forms the predicate of refine.hip's stage B
// (max-subtracted expf, fp32 division, > 0.5f — the mask the refinement loop itself fed back), packs the counts of its four pixels
// into one word per class, and the block reduces: registers -> wavefront (__shfl_down) -> LDS -> one 64-bit atomicAdd per block and
// counter.  Integer sums do not depend on their order: the launch is deterministic.  `n_valid` is read from DEVICE memory, so that
// the ragged last batch of a volume replays the graph that was captured for the full ones.
// HBM-bound: S * K * 4 bytes in per pixel, one byte out (T = 10, batch 8, 256^2: 46 MB in, 0.5 MB out).
#include "matcher.h"

namespace rpnet {

constexpr int kMaxTallySrc = 16;   // sources per launch
struct TallySet { const float* p[kMaxTallySrc]; unsigned char kind[kMaxTallySrc]; };

// class predicted for a pixel with logits l[0 .. K): c >= 1 with softmax(l)[c] > 0.5, else 0 (same expression as refine.hip stage B)
__device__ __forceinline__ int tally_class(const float (&l)[kMaxK], const int K) {
    float mx = l[0];
#pragma unroll
    for (int k = 1; k < kMaxK; ++k)
        if (k < K) mx = fmaxf(mx, l[k]);
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
        if (k < K) den += expf(l[k] - mx);
    int cls = 0;
#pragma unroll
    for (int k = 1; k < kMaxK; ++k)
        if (k < K && expf(l[k] - mx) / den > 0.5f) cls = k;
    return cls;
}

__device__ __forceinline__ unsigned wave_sum_down(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;      // valid in lane 0
}

// counts [S][K-1][3] += {|P and T|, |P|, |T|}; mask [N][H][W] = the class of source mask_src.  A thread = one quad of pixels.
__global__ __launch_bounds__(256) void seg_tally_kernel(const TallySet set, const int S, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ n_valid, unsigned long long* __restrict__ counts,
                                                        uint8_t* __restrict__ mask, const int mask_src, const int N, const int K,
                                                        const unsigned HW, const FastDiv div_hw) {
    RPNET_PASS_PRIORITY();
    // per wave, source and foreground class: |P| in the low half, |P and T| in the high half (a wave holds 256 pixels: 9 bits each)
    __shared__ unsigned part[4][kMaxTallySrc][kMaxK - 1];
    __shared__ unsigned part_t[4][kMaxK - 1];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int nv = min(max(*n_valid, 0), N);
    const unsigned pix = (blockIdx.x * 256u + t) * 4u;           // first pixel of the quad, < N * HW <= 2^32 / K (checked by the launcher)
    unsigned n;
    const unsigned rem = div_hw.divmod(pix, n);                  // HW % 4 == 0: a quad never straddles two images
    const bool live = (unsigned long long)blockIdx.x * 1024ull + t * 4u < (unsigned long long)nv * HW;

    int lab[4] = {-1, -1, -1, -1};
    if (live && labels) {
        const int4 v = *reinterpret_cast<const int4*>(labels + pix);
        lab[0] = v.x; lab[1] = v.y; lab[2] = v.z; lab[3] = v.w;
    }
    if (counts) {
#pragma unroll
        for (int c = 1; c < kMaxK; ++c)
            if (c < K) {
                unsigned tc = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) tc += lab[j] == c ? 1u : 0u;
                tc = wave_sum_down(tc);
                if (lane == 0) part_t[wv][c - 1] = tc;
            }
    }

    for (int s = 0; s < S; ++s) {
        const float* __restrict__ src = set.p[s];
        int cls[4] = {0, 0, 0, 0};
        if (live) {
            if (set.kind[s]) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + pix);
#pragma unroll
                for (int j = 0; j < 4; ++j) cls[j] = v[j] > 0.5f ? 1 : 0;
            } else {
                f32x4 v[kMaxK];
                const float* base = src + (size_t)n * K * HW + rem;
#pragma unroll
                for (int k = 0; k < kMaxK; ++k)
                    if (k < K) v[k] = *reinterpret_cast<const f32x4*>(base + (size_t)k * HW);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float l[kMaxK];
#pragma unroll
                    for (int k = 0; k < kMaxK; ++k) l[k] = k < K ? v[k][j] : 0.f;
                    cls[j] = tally_class(l, K);
                }
            }
            if (mask && s == mask_src)
                *reinterpret_cast<unsigned*>(mask + pix) = (unsigned)cls[0] | (unsigned)cls[1] << 8 | (unsigned)cls[2] << 16 | (unsigned)cls[3] << 24;
        }
        if (counts) {
#pragma unroll
            for (int c = 1; c < kMaxK; ++c)
                if (c < K) {
                    unsigned pc = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) pc += cls[j] == c ? (lab[j] == c ? 0x10001u : 1u) : 0u;
                    pc = wave_sum_down(pc);
                    if (lane == 0) part[wv][s][c - 1] = pc;
                }
        }
    }
    if (!counts) return;
    __syncthreads();
    const int KF = K - 1;
    if (t < S * KF) {
        const int s = t / KF, c = t - s * KF;
        const unsigned a0 = part[0][s][c], a1 = part[1][s][c], a2 = part[2][s][c], a3 = part[3][s][c];
        const unsigned p = (a0 & 0xffffu) + (a1 & 0xffffu) + (a2 & 0xffffu) + (a3 & 0xffffu);
        const unsigned i = (a0 >> 16) + (a1 >> 16) + (a2 >> 16) + (a3 >> 16);
        const unsigned tt = part_t[0][c] + part_t[1][c] + part_t[2][c] + part_t[3][c];
        unsigned long long* dst = counts + ((size_t)s * KF + c) * 3;
        if (i) atomicAdd(dst + 0, (unsigned long long)i);
        if (p) atomicAdd(dst + 1, (unsigned long long)p);
        if (tt) atomicAdd(dst + 2, (unsigned long long)tt);
    }
}

}  // namespace rpnet

extern "C" int rpnet_seg_tally(const float* const* src, const int32_t* src_kind, int S, const int32_t* labels, const int32_t* n_valid,
                               unsigned long long* counts, uint8_t* mask, int mask_src, int N, int K, int H, int W,
                               rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(src && src_kind && n_valid, RPNET_ERR_ARG, "seg_tally: null pointer");
    RPNET_REQUIRE(S >= 1 && S <= kMaxTallySrc, RPNET_ERR_ARG, "seg_tally: %d sources (1..%d per call)", S, kMaxTallySrc);
    RPNET_REQUIRE(K >= 2 && K <= kMaxK, RPNET_ERR_SHAPE, "seg_tally: K=%d (2..%d)", K, kMaxK);
    RPNET_REQUIRE(N >= 0 && H >= 0 && W >= 0 && W % 16 == 0, RPNET_ERR_SHAPE, "seg_tally: N=%d H=%d W=%d (W must be a multiple of 16)", N, H, W);
    RPNET_REQUIRE((counts != nullptr) == (labels != nullptr), RPNET_ERR_ARG, "seg_tally: counts and labels come together");
    const size_t HW = (size_t)H * W;
    if (N == 0 || HW == 0) return RPNET_OK;        // nothing to read (and no FastDiv(0))
    RPNET_REQUIRE(counts || mask, RPNET_ERR_ARG, "seg_tally: neither counts nor a mask to write");
    RPNET_REQUIRE(!mask || (mask_src >= 0 && mask_src < S), RPNET_ERR_ARG, "seg_tally: mask_src=%d of %d sources", mask_src, S);
    RPNET_REQUIRE(((uintptr_t)labels % 16) == 0 && ((uintptr_t)mask % 4) == 0 && ((uintptr_t)counts % 8) == 0, RPNET_ERR_ARG,
                  "seg_tally: labels must be 16-byte, counts 8-byte and mask 4-byte aligned");
    TallySet set{};
    for (int i = 0; i < S; ++i) {
        RPNET_REQUIRE(src[i] && ((uintptr_t)src[i] % 16) == 0, RPNET_ERR_ARG, "seg_tally: source %d is null or not 16-byte aligned", i);
        RPNET_REQUIRE(src_kind[i] == 0 || src_kind[i] == 1, RPNET_ERR_ARG, "seg_tally: source %d has kind %d (0 logits, 1 mask)", i, src_kind[i]);
        set.p[i] = src[i];
        set.kind[i] = (unsigned char)src_kind[i];
    }
    RPNET_REQUIRE((size_t)N * K * HW < kIndex32, RPNET_ERR_SHAPE, "seg_tally: N*K*H*W = %zu does not fit the 32-bit index arithmetic", (size_t)N * K * HW);
    const size_t quads = (size_t)N * HW / 4;
    hipLaunchKernelGGL(seg_tally_kernel, dim3(cdiv((long)quads, 256)), dim3(256), 0, (hipStream_t)stream, set, S, labels, n_valid, counts, mask,
                       mask_src, N, K, (unsigned)HW, FastDiv((unsigned)HW));
    return check_launch("seg_tally");
}
