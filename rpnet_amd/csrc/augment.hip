// Train-time augmentation of the query slices of an episode on the device (rpnet_amd/augment.py; the host restatement is
// rpnet_amd/utils/volume_reader.py: gamma_transform, random_transform, random_label_transform, elastic_transform_all).  Every
// entry point works on ALL slices of a call in one launch, driven by a per-slice parameter table in device memory: an item of k
// slices is two launches for intensity + affine and four for the elastic transform, whatever k.  These are gather kernels on a
// handful of 256 KB slices: what matters is the launch count and that nothing goes back to the host, not bandwidth.
//
//   slice_minmax_kernel    min / max of each slice (registers -> wavefront -> LDS), for the power law and for `lo`
//   augment_affine_kernel  [0,1] map, power law at the SOURCE pixel, nearest sampling through the 2x3 inverse map, zero -> lo
//   blur_axis_kernel       one axis of scipy.ndimage.gaussian_filter (mode reflect) on the two fp64 noise planes, fp64 sums
//   elastic_affine_kernel  stage 1: image bilinear / mask nearest through Minv
//   elastic_warp_kernel    stage 2: image bilinear / mask nearest at (y + dy, x + dx) of the stage-1 result
//
// Coordinates of the elastic stages are fp64 like the host's (the test's tolerance is the host's own change under fp32
// coordinates); the affine stage's are fp32 (its test excludes a band of 1e-3 pixel around the rounding boundaries).
#include "common.h"

namespace rpnet {

constexpr int kAugParams = 8;      // per slice: m00 m01 m02 m10 m11 m12 gamma gamma_on

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// mm [S][2] = {min, max} of x [S][HW]; a block of 1024 threads per slice
__global__ __launch_bounds__(1024) void slice_minmax_kernel(const float* __restrict__ x, float* __restrict__ mm, const int HW) {
    __shared__ float lo_s[16], hi_s[16];
    const float* p = x + (size_t)blockIdx.x * HW;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < HW; i += 1024) {
        const float v = p[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { lo_s[wv] = lo; hi_s[wv] = hi; }
    __syncthreads();
    if (threadIdx.x < 64) {
        lo = wave_min(lo_s[lane & 15]);
        hi = wave_max(hi_s[lane & 15]);
        if (lane == 0) { mm[blockIdx.x * 2] = lo; mm[blockIdx.x * 2 + 1] = hi; }
    }
}

// gamma_transform on one value of the [0,1]-mapped slice.  The law in fp64, rounded once: the host's fp32 formula then differs from
// this by its own rounding error only, which is what the test's tolerance is calibrated on (the cost is nothing at 12 slices).
// Then the host's fp32 round trip between its two functions (gamma_transform returns v * 2 - 1, random_transform takes (x + 1) / 2):
// a value below 3e-8 becomes an exact zero there, and `images == 0` is tested on THAT image.
__device__ __forceinline__ float power_law(const float u, const float lo, const float hi, const float gamma) {
    const double span = (double)hi - (double)lo + 1e-5;
    const float v = (float)(span * pow(((double)u - (double)lo + 1e-5) / span, (double)gamma) + (double)lo);
    return ((v * 2.f - 1.f) + 1.f) / 2.f;
}

// img / lab [S][H][W] -> img_out / lab_out; either pair may be null.  grid (cdiv(HW, 256), S)
__global__ __launch_bounds__(256) void augment_affine_kernel(const float* __restrict__ img, const float* __restrict__ lab,
                                                             const float* __restrict__ params, const float* __restrict__ mm,
                                                             float* __restrict__ img_out, float* __restrict__ lab_out, const int H,
                                                             const int W) {
    const int s = blockIdx.y, HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const float* q = params + s * kAugParams;
    const int y = pix / W, x = pix - y * W;
    // base grid of F.affine_grid in pixels about the centre; grid_sample(align_corners=False) un-normalises to sx + W/2 - 1/2
    const float bx = (float)x - 0.5f * W + 0.5f, by = (float)y - 0.5f * H + 0.5f;
    const float fx = fmaf(q[0], bx, fmaf(q[1], by, q[2])) + (0.5f * W - 0.5f);
    const float fy = fmaf(q[3], bx, fmaf(q[4], by, q[5])) + (0.5f * H - 0.5f);
    const float rx = rintf(fx), ry = rintf(fy);        // round half to even, as nearbyint
    const bool inside = rx >= 0.f && rx <= (float)(W - 1) && ry >= 0.f && ry <= (float)(H - 1);
    const size_t src = (size_t)s * HW + (inside ? (int)ry * W + (int)rx : 0);
    const size_t dst = (size_t)s * HW + pix;
    if (lab_out) lab_out[dst] = inside ? lab[src] : 0.f;
    if (img_out) {
        const float lo_u = (mm[2 * s] + 1.f) / 2.f, hi_u = (mm[2 * s + 1] + 1.f) / 2.f;
        const bool g = q[7] != 0.f;
        // `lo`: the minimum of the [0,1] image the sampling stage is given; the power law is monotone, so it is the law's value
        // at the slice minimum
        const float lo = g ? power_law(lo_u, lo_u, hi_u, q[6]) : lo_u;
        float v = 0.f;
        if (inside) {
            v = (img[src] + 1.f) / 2.f;
            if (g) v = power_law(v, lo_u, hi_u, q[6]);
        }
        if (v == 0.f) v = lo;      // zeros of the [0,1] image the sampling stage was given (after the round trip above), and the fill
        img_out[dst] = v * 2.f - 1.f;
    }
}

// index of the reflect extension (d c b a | a b c d | d c b a), periodic with period 2n
__device__ __forceinline__ int reflect(int i, const int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// out[c][y][x] = scale * sum_t w[t] in[c][.. + t - r ..] along `axis` (0: y, 1: x); fp64.  grid (cdiv(HW, 256), planes)
template <typename OutT>
__global__ __launch_bounds__(256) void blur_axis_kernel(const double* __restrict__ in, const double* __restrict__ w, OutT* __restrict__ out,
                                                        const int H, const int W, const int radius, const int axis, const double scale) {
    const int HW = H * W, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const double* p = in + (size_t)blockIdx.y * HW;
    const int y = pix / W, x = pix - y * W;
    double acc = 0.0;
    if (axis == 0) {
        for (int t = -radius; t <= radius; ++t) acc += w[t + radius] * p[reflect(y + t, H) * W + x];
    } else {
        for (int t = -radius; t <= radius; ++t) acc += w[t + radius] * p[y * W + reflect(x + t, W)];
    }
    out[(size_t)blockIdx.y * HW + pix] = (OutT)(acc * scale);
}

struct Affine64 { double m[6]; };

// scipy.ndimage.map_coordinates(order=1, mode="constant") at (cy, cx): a coordinate outside [0, n-1] gives cval, no blending
__device__ __forceinline__ float bilinear_const(const float* __restrict__ p, const int H, const int W, const double cy, const double cx,
                                                const float cval) {
    if (!(cy >= 0.0 && cy <= (double)(H - 1) && cx >= 0.0 && cx <= (double)(W - 1))) return cval;
    const double fy = floor(cy), fx = floor(cx);
    const int y0 = (int)fy, x0 = (int)fx;
    const double wy = cy - fy, wx = cx - fx;
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);      // a tap past the edge has weight zero
    const double top = (1.0 - wx) * (double)p[y0 * W + x0] + wx * (double)p[y0 * W + x1];
    const double bot = (1.0 - wx) * (double)p[y1 * W + x0] + wx * (double)p[y1 * W + x1];
    return (float)((1.0 - wy) * top + wy * bot);
}

// stage 1: image bilinear at Minv p, mask nearest at rint(Minv p) (half to even, numpy.rint).  grid (cdiv(HW, 256), S)
__global__ __launch_bounds__(256) void elastic_affine_kernel(const float* __restrict__ img, const float* __restrict__ mask, const Affine64 A,
                                                             float* __restrict__ img_out, float* __restrict__ mask_out, const int H,
                                                             const int W, const float cval) {
    const int HW = H * W, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int y = pix / W, x = pix - y * W;
    const size_t base = (size_t)blockIdx.y * HW;
    // the host's order of operations, unfused, so that the mask's rounding sees the same fp64 number
    const double sx = __dadd_rn(__dadd_rn(__dmul_rn(A.m[0], (double)x), __dmul_rn(A.m[1], (double)y)), A.m[2]);
    const double sy = __dadd_rn(__dadd_rn(__dmul_rn(A.m[3], (double)x), __dmul_rn(A.m[4], (double)y)), A.m[5]);
    if (img_out) img_out[base + pix] = bilinear_const(img + base, H, W, sy, sx, cval);
    if (mask_out) {
        const double rx = rint(sx), ry = rint(sy);
        const bool inside = rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1);
        mask_out[base + pix] = inside ? mask[base + (int)ry * W + (int)rx] : 0.f;
    }
}

// stage 2: field [2][H][W] = (dx, dy); image bilinear, mask order 0 (floor(c + 0.5), outside [0, n-1] zero) at (y + dy, x + dx)
__global__ __launch_bounds__(256) void elastic_warp_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                                           const float* __restrict__ field, float* __restrict__ img_out,
                                                           float* __restrict__ mask_out, const int H, const int W, const float cval) {
    const int HW = H * W, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int y = pix / W, x = pix - y * W;
    const size_t base = (size_t)blockIdx.y * HW;
    const double cx = (double)x + (double)field[pix], cy = (double)y + (double)field[HW + pix];
    if (img_out) img_out[base + pix] = bilinear_const(img + base, H, W, cy, cx, cval);
    if (mask_out) {
        const bool inside = cy >= 0.0 && cy <= (double)(H - 1) && cx >= 0.0 && cx <= (double)(W - 1);
        mask_out[base + pix] = inside ? mask[base + (int)floor(cy + 0.5) * W + (int)floor(cx + 0.5)] : 0.f;
    }
}

static int check_plane(const char* what, int S, int H, int W) {
    RPNET_REQUIRE(S >= 0 && H >= 1 && W >= 1, RPNET_ERR_SHAPE, "%s: S=%d H=%d W=%d", what, S, H, W);
    RPNET_REQUIRE(S <= 65535, RPNET_ERR_SHAPE, "%s: %d slices (at most 65535 per call)", what, S);
    RPNET_REQUIRE((size_t)(S ? S : 1) * H * W < ((size_t)1 << 31), RPNET_ERR_SHAPE, "%s: S*H*W does not fit the 32-bit index arithmetic", what);
    return RPNET_OK;
}

}  // namespace rpnet

extern "C" int rpnet_slice_minmax(const float* x, float* mm, int S, int H, int W, rpnet_stream_t stream) {
    using namespace rpnet;
    if (int rc = check_plane("slice_minmax", S, H, W)) return rc;
    if (S == 0) return RPNET_OK;
    RPNET_REQUIRE(x && mm, RPNET_ERR_ARG, "slice_minmax: null pointer");
    hipLaunchKernelGGL(slice_minmax_kernel, dim3(S), dim3(1024), 0, (hipStream_t)stream, x, mm, H * W);
    return check_launch("slice_minmax");
}

extern "C" int rpnet_augment_affine(const float* img, const float* lab, const float* params, const float* mm, float* img_out,
                                    float* lab_out, int S, int H, int W, rpnet_stream_t stream) {
    using namespace rpnet;
    if (int rc = check_plane("augment_affine", S, H, W)) return rc;
    if (S == 0) return RPNET_OK;
    RPNET_REQUIRE(params, RPNET_ERR_ARG, "augment_affine: null parameter table");
    RPNET_REQUIRE((img != nullptr) == (img_out != nullptr) && (lab != nullptr) == (lab_out != nullptr) && (img || lab), RPNET_ERR_ARG,
                  "augment_affine: an input and its output come together, and at least one pair");
    RPNET_REQUIRE(!img || mm, RPNET_ERR_ARG, "augment_affine: images need the min/max table of rpnet_slice_minmax");
    RPNET_REQUIRE((!img || img != img_out) && (!lab || lab != lab_out), RPNET_ERR_ARG, "augment_affine: a gather cannot run in place");
    hipLaunchKernelGGL(augment_affine_kernel, dim3(cdiv((long)H * W, 256), S), dim3(256), 0, (hipStream_t)stream, img, lab, params, mm,
                       img_out, lab_out, H, W);
    return check_launch("augment_affine");
}

extern "C" int rpnet_elastic_field(const double* noise, const double* weights, int radius, double alpha, double* tmp, float* field, int H,
                                   int W, rpnet_stream_t stream) {
    using namespace rpnet;
    if (int rc = check_plane("elastic_field", 2, H, W)) return rc;
    RPNET_REQUIRE(noise && weights && tmp && field, RPNET_ERR_ARG, "elastic_field: null pointer");
    RPNET_REQUIRE(radius >= 0 && radius < (1 << 20), RPNET_ERR_ARG, "elastic_field: radius %d", radius);
    RPNET_REQUIRE(noise != tmp, RPNET_ERR_ARG, "elastic_field: tmp must not alias the noise planes");
    const dim3 grid(cdiv((long)H * W, 256), 2);
    hipLaunchKernelGGL(blur_axis_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, noise, weights, tmp, H, W, radius, 0, 1.0);
    hipLaunchKernelGGL(blur_axis_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)tmp, weights, field, H, W, radius, 1,
                       alpha);
    return check_launch("elastic_field");
}

extern "C" int rpnet_elastic_apply(const float* img, const float* mask, const double* minv, const float* field, float* img_tmp,
                                   float* mask_tmp, float* img_out, float* mask_out, int S, int H, int W, float padding_value,
                                   rpnet_stream_t stream) {
    using namespace rpnet;
    if (int rc = check_plane("elastic_apply", S, H, W)) return rc;
    if (S == 0) return RPNET_OK;
    RPNET_REQUIRE(minv && field, RPNET_ERR_ARG, "elastic_apply: null Minv or field");
    RPNET_REQUIRE((img != nullptr) == (img_out != nullptr) && (img != nullptr) == (img_tmp != nullptr), RPNET_ERR_ARG,
                  "elastic_apply: image, its intermediate and its output come together");
    RPNET_REQUIRE((mask != nullptr) == (mask_out != nullptr) && (mask != nullptr) == (mask_tmp != nullptr), RPNET_ERR_ARG,
                  "elastic_apply: mask, its intermediate and its output come together");
    RPNET_REQUIRE(img || mask, RPNET_ERR_ARG, "elastic_apply: neither images nor masks");
    RPNET_REQUIRE((!img || (img != img_tmp && img_tmp != img_out)) && (!mask || (mask != mask_tmp && mask_tmp != mask_out)), RPNET_ERR_ARG,
                  "elastic_apply: a gather cannot run in place");
    Affine64 A;
    for (int i = 0; i < 6; ++i) A.m[i] = minv[i];          // HOST pointer: six numbers, passed by value
    const dim3 grid(cdiv((long)H * W, 256), S);
    hipLaunchKernelGGL(elastic_affine_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, mask, A, img_tmp, mask_tmp, H, W, padding_value);
    hipLaunchKernelGGL(elastic_warp_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)img_tmp, (const float*)mask_tmp, field,
                       img_out, mask_out, H, W, padding_value);
    return check_launch("elastic_apply");
}
