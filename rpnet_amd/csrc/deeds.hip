// DEEDS registration of the reader's slices (net/registration.py:360-381,412-471; include/rpnet_deeds_abi.h): one pass, no optimiser.
// A cost per grid point (G x G) and displacement (D x D), regularised twice, then a softmax expectation of the displacements.
//
// In torch the cost volume (G^2 D^2 floats per slice: 14.7 MB at 128^2 x 15^2) goes through memory about ten times.  Here it never
// reaches HBM on the default path (alpha3 == 0).  A block owns T x T grid points and the ring of 2 around them, (T + 4)^2 points, and
// keeps their D^2 costs in LDS:
//   fill      cost[p][d] = alpha1 + alpha0 (fixed(grid_p) - moving(grid_p + shift_d))^2, bilinear samples with zero padding
//   minconv   per point, over its displacement plane: replicate pad 3, 3x3 min, two 3x3 averages, back into the plane (a wave per point,
//             two scratch planes of (D + 4)^2 and (D + 2)^2 floats per wave)
//   meanfield per inner point and displacement, over the grid plane: replicate pad 2 and two 3x3 averages are one 5x5 filter with the
//             taps (1 2 3 2 1) x (1 2 3 2 1) / 81 over indices clamped to the grid
//   softmax   over the D^2 values of an inner point, held in the registers of one wave (at most 16 per lane), maximum subtracted first
// Only points inside the grid are stored and computed; a neighbour outside it is the clamped index, which is what replicate padding
// means.  T is chosen by the host from D so that the tile fits the 160 KiB of a CU (deeds_plan): 8 for D <= 15.
// alpha3 != 0 needs the first path's mean field at the ring as well: the same kernel runs twice, the first launch writes its mean field
// to a workspace (chunked over slices), the second adds it to its costs.
// No atomics, no block waits for another, every loop runs to a count fixed when it is entered; the wave reductions are butterflies, so
// two runs give the same bits.
#include <math.h>

#include "common.h"
#include "rpnet_deeds_abi.h"

namespace rpnet {
namespace {

constexpr int kDeedsLds = 160 * 1024;       // LDS of a gfx950 CU, all of which one block may take
constexpr int kDeedsMaxTile = 8;
constexpr int kDeedsRegs = 16;              // ceil(31^2 / 64): the costs of a point in the registers of a wave
constexpr size_t kDeedsChunkBytes = (size_t)1 << 28;
constexpr int kDeedsMaxSlices = 32768;      // slices of one launch (gridDim.y)

struct DeedsPlan {
    int tile, waves;
    size_t lds;
};

// the largest tile T <= 8, then the most waves (8, 4, 2, 1), whose (T + 4)^2 (D^2 + 1) costs and per-wave scratch fit the LDS
static DeedsPlan deeds_plan(int D) {
    const size_t dd = (size_t)D * D, scratch = (size_t)(D + 4) * (D + 4) + (size_t)(D + 2) * (D + 2);
    for (int t = kDeedsMaxTile; t >= 1; --t)
        for (int w = 8; w >= 1; w >>= 1) {
            const size_t lds = ((size_t)(t + 4) * (t + 4) * (dd + 1) + (size_t)w * scratch) * sizeof(float);
            if (lds <= (size_t)kDeedsLds) return {t, w, lds};
        }
    return {0, 0, 0};
}

__device__ __forceinline__ float deeds_sample(const float* __restrict__ img, int H, int W, float gx, float gy) {
    const float ix = (gx + 1.f) * (0.5f * (float)W) - 0.5f, iy = (gy + 1.f) * (0.5f * (float)H) - 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = sample_cell(fx, W), y0 = sample_cell(fy, H);
    const float tx = ix - fx, ty = iy - fy;
    const bool xin0 = x0 >= 0 && x0 < W, xin1 = x0 + 1 >= 0 && x0 + 1 < W;
    const bool yin0 = y0 >= 0 && y0 < H, yin1 = y0 + 1 >= 0 && y0 + 1 < H;
    const float nw = (xin0 && yin0) ? img[y0 * W + x0] : 0.f;
    const float ne = (xin1 && yin0) ? img[y0 * W + x0 + 1] : 0.f;
    const float sw = (xin0 && yin1) ? img[(y0 + 1) * W + x0] : 0.f;
    const float se = (xin1 && yin1) ? img[(y0 + 1) * W + x0 + 1] : 0.f;
    return nw * (1.f - tx) * (1.f - ty) + ne * tx * (1.f - ty) + sw * (1.f - tx) * ty + se * tx * ty;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// MODE 0: alpha3 == 0, cost = alpha4 + alpha2 dc, regularised once, softmax.  MODE 1: cost = dc, its mean field goes to ws.
// MODE 2: cost = alpha4 + alpha2 dc + alpha3 ws, regularised, softmax.
template <int MODE>
__global__ __launch_bounds__(512) void deeds_kernel(const float* __restrict__ moving, const float* __restrict__ fixed,
                                                     const float* __restrict__ gbase, const float* __restrict__ sbase, const int H,
                                                     const int W, const int G, const int D, const int T, const float range,
                                                     const float a0, const float a1, const float a2, const float a3, const float a4,
                                                     const float a5, float* __restrict__ ws, float* __restrict__ pred,
                                                     float* __restrict__ cost_out) {
    extern __shared__ __attribute__((aligned(16))) float deeds_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const int DD = D * D, RW = T + 4, NR = RW * RW;
    const int tiles = (G + T - 1) / T;
    const int by = blockIdx.x / tiles, bx = blockIdx.x - by * tiles;
    const int oy = by * T - 2, ox = bx * T - 2;             // grid point of region slot (0, 0)
    const size_t slice = blockIdx.y;
    const float* mov = moving + slice * (size_t)H * W;
    const float* fix = fixed + slice * (size_t)H * W;
    float* cost = deeds_lds;                                // [NR][DD]
    float* fval = cost + (size_t)NR * DD;                   // [NR] fixed(grid_p)
    const int MW = D + 4, AW = D + 2;
    float* mpl = fval + NR + (size_t)wv * (MW * MW + AW * AW);      // this wave's [MW][MW] minima
    float* apl = mpl + MW * MW;                                     // this wave's [AW][AW] first averages

    for (int p = tid; p < NR; p += blockDim.x) {
        const int ry = p / RW, gy = oy + ry, gx = ox + p - ry * RW;
        fval[p] = (gy >= 0 && gy < G && gx >= 0 && gx < G) ? deeds_sample(fix, H, W, gbase[gx], gbase[gy]) : 0.f;
    }
    __syncthreads();

    // fill: a wave per point, its lanes over the displacements
    for (int p = wv; p < NR; p += nw) {
        const int ry = p / RW, gy = oy + ry, gx = ox + p - ry * RW;
        if (gy < 0 || gy >= G || gx < 0 || gx >= G) continue;
        const float px = gbase[gx], py = gbase[gy], f = fval[p];
        const size_t wrow = (slice * (size_t)G * G + (size_t)gy * G + gx) * DD;
        for (int d = lane; d < DD; d += 64) {
            const int di = d / D, dj = d - di * D;
            const float m = deeds_sample(mov, H, W, px + sbase[dj] * range, py + sbase[di] * range);
            const float diff = f - m;
            float c = a1 + a0 * (diff * diff);
            if (MODE == 0) c = a4 + a2 * c;
            if (MODE == 2) c = a4 + a2 * c + a3 * ws[wrow + d];
            cost[(size_t)p * DD + d] = c;
        }
    }
    __syncthreads();

    // minconv: the waves go through their points in step, so the three barriers of a round are met by all
    const int rounds = (NR + nw - 1) / nw;
    for (int r = 0; r < rounds; ++r) {
        const int p = r * nw + wv;
        const int ry = p / RW, gy = oy + ry, gx = ox + p - ry * RW;
        const bool live = p < NR && gy >= 0 && gy < G && gx >= 0 && gx < G;
        float* c = cost + (size_t)(live ? p : 0) * DD;
        if (live)
            for (int e = lane; e < MW * MW; e += 64) {
                const int i = e / MW, j = e - i * MW;           // plane position (i - 2, j - 2) of the padded minimum
                float m = INFINITY;
#pragma unroll
                for (int a = -1; a <= 1; ++a) {
                    const int ci = clampi(i - 2 + a, 0, D - 1) * D;
#pragma unroll
                    for (int b = -1; b <= 1; ++b) m = fminf(m, c[ci + clampi(j - 2 + b, 0, D - 1)]);
                }
                mpl[e] = m;
            }
        __syncthreads();
        if (live)
            for (int e = lane; e < AW * AW; e += 64) {
                const int i = e / AW, j = e - i * AW;
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) s += mpl[(i + a) * MW + j + b];
                apl[e] = s / 9.f;
            }
        __syncthreads();
        if (live)
            for (int e = lane; e < DD; e += 64) {
                const int i = e / D, j = e - i * D;
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) s += apl[(i + a) * AW + j + b];
                c[e] = s / 9.f;
            }
        __syncthreads();
    }

    // mean field and softmax: a wave per inner point
    for (int q = wv; q < T * T; q += nw) {
        const int ty = q / T, gy = by * T + ty, gx = bx * T + q - ty * T;
        if (gy >= G || gx >= G) continue;
        int rowoff[5], coloff[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            rowoff[k] = (clampi(gy + k - 2, 0, G - 1) - oy) * RW;
            coloff[k] = clampi(gx + k - 2, 0, G - 1) - ox;
        }
        float v[kDeedsRegs];
        const size_t point = slice * (size_t)G * G + (size_t)gy * G + gx;
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < kDeedsRegs; ++k) {
            const int d = k * 64 + lane;
            v[k] = 0.f;
            if (d < DD) {
                float tot = 0.f;
#pragma unroll
                for (int a = 0; a < 5; ++a) {
                    const float* row = cost + (size_t)rowoff[a] * DD + d;
                    const float rs = (row[(size_t)coloff[0] * DD] + row[(size_t)coloff[4] * DD]) +
                                     2.f * (row[(size_t)coloff[1] * DD] + row[(size_t)coloff[3] * DD]) + 3.f * row[(size_t)coloff[2] * DD];
                    tot += (a == 2 ? 3.f : (a == 1 || a == 3 ? 2.f : 1.f)) * rs;
                }
                v[k] = tot / 81.f;
                if (MODE == 1) ws[point * DD + d] = v[k];
                if (MODE != 1 && cost_out) cost_out[point * DD + d] = v[k];
                if (MODE != 1) mx = fmaxf(mx, -a5 * v[k]);
            }
        }
        if (MODE == 1) continue;
        mx = wave_max(mx);
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < kDeedsRegs; ++k) {
            const int d = k * 64 + lane;
            v[k] = d < DD ? expf(-a5 * v[k] - mx) : 0.f;
            se += v[k];
        }
        se = wave_sum(se);
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int k = 0; k < kDeedsRegs; ++k) {
            const int d = k * 64 + lane;
            if (d < DD) {
                const int di = d / D, dj = d - di * D;
                const float w = v[k] / se;
                sx += w * (sbase[dj] * range);
                sy += w * (sbase[di] * range);
            }
        }
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        if (lane == 0) {
            pred[point * 2] = sx;
            pred[point * 2 + 1] = sy;
        }
    }
}

// the sampling grid (grid + pred) [G][G][2] brought to H x W by torch's legacy `nearest` rule or by `bilinear` (align_corners=False),
// then out = [threshold](scale * sample(x) + shift) as warp_kernel of registration.hip
template <int MODE>
__global__ __launch_bounds__(256) void deeds_warp_kernel(const float* __restrict__ x, const float* __restrict__ pred,
                                                          const float* __restrict__ gbase, float* __restrict__ out, const int H,
                                                          const int W, const int G, const float threshold, const float scale,
                                                          const float shift) {
    const int HW = H * W;
    const float* img = x + (size_t)blockIdx.y * HW;
    const float* pr = pred + (size_t)blockIdx.y * G * G * 2;
    const float sh = (float)G / (float)H, sw = (float)G / (float)W;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        const int i = p / W, j = p - i * W;
        float gx, gy;
        if (MODE == 0) {
            const int si = min((int)floorf((float)i * sh), G - 1), sj = min((int)floorf((float)j * sw), G - 1);
            const float* q = pr + ((size_t)si * G + sj) * 2;
            gx = gbase[sj] + q[0];
            gy = gbase[si] + q[1];
        } else {
            const float fy = fmaxf(sh * ((float)i + 0.5f) - 0.5f, 0.f), fx = fmaxf(sw * ((float)j + 0.5f) - 0.5f, 0.f);
            const int i0 = min((int)fy, G - 1), j0 = min((int)fx, G - 1);
            const int i1 = i0 + (i0 < G - 1 ? 1 : 0), j1 = j0 + (j0 < G - 1 ? 1 : 0);
            const float ly1 = fy - (float)i0, ly0 = 1.f - ly1, lx1 = fx - (float)j0, lx0 = 1.f - lx1;
            const float* q00 = pr + ((size_t)i0 * G + j0) * 2;
            const float* q01 = pr + ((size_t)i0 * G + j1) * 2;
            const float* q10 = pr + ((size_t)i1 * G + j0) * 2;
            const float* q11 = pr + ((size_t)i1 * G + j1) * 2;
            const float bx0 = gbase[j0], bx1 = gbase[j1], by0 = gbase[i0], by1 = gbase[i1];
            gx = ly0 * (lx0 * (bx0 + q00[0]) + lx1 * (bx1 + q01[0])) + ly1 * (lx0 * (bx0 + q10[0]) + lx1 * (bx1 + q11[0]));
            gy = ly0 * (lx0 * (by0 + q00[1]) + lx1 * (by0 + q01[1])) + ly1 * (lx0 * (by1 + q10[1]) + lx1 * (by1 + q11[1]));
        }
        float v = deeds_sample(img, H, W, gx, gy);
        if (threshold >= 0.f) v = v > threshold ? 1.f : 0.f;
        out[(size_t)blockIdx.y * HW + p] = v * scale + shift;
    }
}

static bool deeds_dims_ok(int G, int D) { return G >= 1 && G <= RPNET_DEEDS_MAX_GRID && D >= 1 && D <= RPNET_DEEDS_MAX_WIDTH && (D & 1); }

static size_t deeds_chunk(int S, int G, int D) {
    const size_t per = (size_t)G * G * D * D * sizeof(float);
    size_t chunk = kDeedsChunkBytes / per;
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)kDeedsMaxSlices) chunk = kDeedsMaxSlices;
    return chunk < (size_t)S ? chunk : (size_t)S;
}

template <int MODE>
static void deeds_launch(const DeedsPlan& plan, int n, hipStream_t s, const float* moving, const float* fixed, const float* gbase,
                         const float* sbase, int H, int W, int G, int D, float range, const float* al, float* ws, float* pred,
                         float* cost_out) {
    const int tiles = cdiv(G, plan.tile);
    if (plan.lds > 64 * 1024)      // more than 64 KiB of dynamic LDS needs the opt-in (gfx950 has 160 KiB per CU)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&deeds_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds);
    hipLaunchKernelGGL((deeds_kernel<MODE>), dim3(tiles * tiles, n), dim3(plan.waves * 64), plan.lds, s, moving, fixed, gbase, sbase, H, W,
                       G, D, plan.tile, range, al[0], al[1], al[2], al[3], al[4], al[5], ws, pred, cost_out);
}

}  // namespace
}  // namespace rpnet

extern "C" int rpnet_deeds_abi_version(void) { return RPNET_DEEDS_ABI_VERSION; }

extern "C" size_t rpnet_deeds_workspace_bytes(int S, int G, int D, int general) {
    using namespace rpnet;
    if (S < 0 || !deeds_dims_ok(G, D)) {
        set_error("deeds_workspace_bytes: S=%d G=%d D=%d (S >= 0, G 1..%d, D odd 1..%d)", S, G, D, RPNET_DEEDS_MAX_GRID, RPNET_DEEDS_MAX_WIDTH);
        return 0;
    }
    if (!general || S == 0) return 0;
    return deeds_chunk(S, G, D) * (size_t)G * G * D * D * sizeof(float);
}

extern "C" int rpnet_deeds_register(const float* moving, const float* fixed, const float* gbase, const float* sbase, int S, int H, int W,
                                    int G, int D, float disp_range, float alpha0, float alpha1, float alpha2, float alpha3, float alpha4,
                                    float alpha5, float* pred, float* cost_out, void* ws, size_t ws_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(moving && fixed && gbase && sbase && pred, RPNET_ERR_ARG, "deeds_register: null pointer");
    RPNET_REQUIRE(S >= 0 && H >= 2 && W >= 2 && (long)H * W < (1L << 30), RPNET_ERR_SHAPE, "deeds_register: S=%d H=%d W=%d", S, H, W);
    RPNET_REQUIRE(deeds_dims_ok(G, D), RPNET_ERR_SHAPE, "deeds_register: G=%d D=%d (G 1..%d, D odd 1..%d)", G, D, RPNET_DEEDS_MAX_GRID,
                  RPNET_DEEDS_MAX_WIDTH);
    const float al[6] = {alpha0, alpha1, alpha2, alpha3, alpha4, alpha5};
    bool finite = isfinite(disp_range);
    for (int k = 0; k < 6; ++k) finite = finite && isfinite(al[k]);
    RPNET_REQUIRE(finite, RPNET_ERR_ARG, "deeds_register: disp_range or alpha is not finite");
    const bool general = alpha3 != 0.f;
    const size_t need = rpnet_deeds_workspace_bytes(S, G, D, general);
    RPNET_REQUIRE(need == 0 || (ws && ws_bytes >= need), RPNET_ERR_ARG, "deeds_register: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0,
                  need);
    if (S == 0) return RPNET_OK;
    const DeedsPlan plan = deeds_plan(D);
    const size_t chunk = general ? deeds_chunk(S, G, D) : (size_t)kDeedsMaxSlices;
    const size_t GG = (size_t)G * G, HW = (size_t)H * W, DD = (size_t)D * D;
    hipStream_t s = (hipStream_t)stream;
    for (size_t s0 = 0; s0 < (size_t)S; s0 += chunk) {
        const int n = (int)((size_t)S - s0 < chunk ? (size_t)S - s0 : chunk);
        const float *m = moving + s0 * HW, *f = fixed + s0 * HW;
        float* p = pred + s0 * GG * 2;
        float* c = cost_out ? cost_out + s0 * GG * DD : nullptr;
        if (general) {
            deeds_launch<1>(plan, n, s, m, f, gbase, sbase, H, W, G, D, disp_range, al, (float*)ws, p, c);
            deeds_launch<2>(plan, n, s, m, f, gbase, sbase, H, W, G, D, disp_range, al, (float*)ws, p, c);
        } else {
            deeds_launch<0>(plan, n, s, m, f, gbase, sbase, H, W, G, D, disp_range, al, nullptr, p, c);
        }
    }
    return check_launch("deeds_register");
}

extern "C" int rpnet_deeds_warp(const float* x, const float* pred, const float* gbase, float* out, int S, int H, int W, int G, int mode,
                                float threshold, float scale, float shift, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(x && pred && gbase && out, RPNET_ERR_ARG, "deeds_warp: null pointer");
    RPNET_REQUIRE(S >= 0 && H >= 2 && W >= 2 && (long)H * W < (1L << 30), RPNET_ERR_SHAPE, "deeds_warp: S=%d H=%d W=%d", S, H, W);
    RPNET_REQUIRE(G >= 1 && G <= RPNET_DEEDS_MAX_GRID, RPNET_ERR_SHAPE, "deeds_warp: G=%d (1..%d)", G, RPNET_DEEDS_MAX_GRID);
    RPNET_REQUIRE(mode == RPNET_DEEDS_NEAREST || mode == RPNET_DEEDS_BILINEAR, RPNET_ERR_ARG, "deeds_warp: mode=%d (0 nearest, 1 bilinear)", mode);
    hipStream_t s = (hipStream_t)stream;
    for (int s0 = 0; s0 < S; s0 += kDeedsMaxSlices) {
        const int n = S - s0 < kDeedsMaxSlices ? S - s0 : kDeedsMaxSlices;
        const dim3 grid(cdiv((long)H * W, 256 * 4), n);
        const float* xi = x + (size_t)s0 * H * W;
        const float* pi = pred + (size_t)s0 * G * G * 2;
        float* oi = out + (size_t)s0 * H * W;
        if (mode == RPNET_DEEDS_NEAREST)
            hipLaunchKernelGGL(deeds_warp_kernel<0>, grid, dim3(256), 0, s, xi, pi, gbase, oi, H, W, G, threshold, scale, shift);
        else
            hipLaunchKernelGGL(deeds_warp_kernel<1>, grid, dim3(256), 0, s, xi, pi, gbase, oi, H, W, G, threshold, scale, shift);
    }
    return check_launch("deeds_warp");
}
