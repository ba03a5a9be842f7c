// Separable Gaussian smoothing of a [D][H][W] float32 or int16 volume (include/rpnet_smooth_abi.h; rpnet_amd/smooth.py): the device form
// of scipy.ndimage.gaussian_filter and the prefilter of a shrinking resample.
//
// What was chosen.  One launch per axis whose radius is not 0, x then y then z, with float64 intermediates in the workspace: the first
// pass reads the volume's kind, the last writes it, so three passes move 4 + 8 + 8 + 8 + 8 + 4 = 40 B per float32 voxel, two move 24 and
// one moves 8.  That is the plain byte account, not the fused one (x and y on one slice tile in LDS: 24 B; a ring of filtered slices
// down z: towards 8 B).  The fused kernels hold a halo of 2r rows or slices per tile, so they fit LDS only for small radii and
// would stand beside these three passes, which every radius up to 255 needs anyway; this file is the one path that is right for every
// radius, and the fused one is left to be added on top of it when its gain has been measured.  profiles/smooth.txt has the rates of this
// one against its own byte account, pass by pass: at radius 3 the x / y / z passes of a 64 x 512 x 512 float32 volume run at 2.8 / 4.8 /
// 4.4 TB/s of the bytes they move, and at radius 32 every pass takes about 3.2 times as long for the same bytes, the z pass no more than
// the x pass: the time there is the tap loop's.
// Within a pass a tap is meant to cross HBM once; for the x pass that holds by construction, for the y and z passes it rests on the caches
// (the trace above does not contradict it, and no counter has been read to confirm it):
//  - x pass: a block is 4 waves, a wave owns 64 runs of one row (256 float32, 512 int16).  It stages the segment and its halo of r voxels
//    on either side in LDS as float64, its own run with one 16-byte load per lane and the halo element by element with the index folded;
//    only the halo is folded, the interior is not.  A lane then walks the 2r + R positions its R outputs need once, holding the R sums in
//    registers.  Lane l starts at position l * R, a stride of 8 * R bytes, which would put lanes l and l + 64 / (2 * R) on one bank:
//    position e is stored at e + e / 32, one float64 of padding per 32, and the 32 lanes that a ds_read_b64 serves together then fall on
//    32 different bank pairs for R = 4 and for R = 8.
//  - y and z passes: the volume is [outer][n][inner] with the pass along n (y: [D][H][W]; z: [1][D][H * W]).  A lane owns a run of R
//    consecutive inner positions and kSmoothSegVoxels / R consecutive outputs along n, and walks the rows its outputs need once, from
//    global memory into registers: neighbouring lanes read neighbouring runs, so a wave reads whole rows 16 bytes (or 8 * R bytes of
//    float64) per lane at a time, and a row is fetched by ceil((seg + 2r) / seg) lanes that run side by side and are expected to meet in
//    L2 (the lanes of one row stand in neighbouring blocks, which the dispatcher spreads over the XCDs, so some of these re-reads go past
//    an L2 to the Infinity Cache).  There is no LDS tile in these passes, so no column of an LDS tile to conflict on.  The index along n
//    is folded once per row of the walk and only where it leaves the line.
//  - The weights, at most 511 float64, are read once per block into LDS; every lane of a wave reads the same one (a broadcast), and a
//    lane keeps the weights its sums are at in a register window that shifts by one per step.
// The sum of the definition is spelled one rounding at a time, ascending in k for every output (a lane meets the taps of an output in
// ascending order, since it walks its positions in ascending order), and the file is built with -ffp-contract=off: a numpy restatement
// gets the same bits.  A tap outside an output's window is skipped by a predicate that is uniform over the block, never multiplied by 0.
//
// Bounds: every index that is read has gone through smooth_fold (or lies inside the line), and a run reads and writes only its `cnt`
// elements; a wave whose row lies behind the last row reads the last row and stores nothing; a lane beyond the last run does nothing.
// Every loop runs to a count fixed when it is entered.  No atomics.
#include <cmath>

#include "cc_phases.h"
#include "rpnet_smooth_abi.h"

namespace rpnet {

constexpr int kSmoothRunBytes = 16;                 // bytes of the volume's kind a lane owns along x
constexpr int kSmoothXRows = 4;                     // rows of a block of the x pass, one per wave
constexpr int kSmoothSegVoxels = 32;                // outputs of a lane of the y and z passes: R along the row times 32 / R along the axis
constexpr int kSmoothMaxTaps = 2 * RPNET_SMOOTH_MAX_RADIUS + 1;
__host__ __device__ constexpr int smooth_pad(const int e) { return e + (e >> 5); }
constexpr int kSmoothPitch = smooth_pad(64 * 8 + 2 * RPNET_SMOOTH_MAX_RADIUS) + 1;    // float64 of a staged row, int16 runs, radius 255

__device__ __forceinline__ int smooth_fold(const int j, const int n, const int border) {
    if (border == RPNET_SMOOTH_NEAREST) return min(max(j, 0), n - 1);
    const int p = 2 * n;
    int m = j % p;
    if (m < 0) m += p;
    return m >= n ? p - 1 - m : m;
}

// the one conversion of a result to the output kind; a float64 intermediate is not converted
__device__ __forceinline__ double smooth_convert(const double r, double) { return r; }
__device__ __forceinline__ float smooth_convert(const double r, float) { return (float)r; }
__device__ __forceinline__ int16_t smooth_convert(const double r, int16_t) {
    return (int16_t)(int)fmin(fmax(rint(r), -32768.0), 32767.0);              // rint: half to even
}

// v[0..R) = p[0..cnt) widened, 0 behind cnt: 16-byte loads where the run is whole and aligned
template <class T, int R>
__device__ __forceinline__ void smooth_load_run(const T* __restrict__ p, const int cnt, double (&v)[R]) {
    constexpr int kVec = 16 / (int)sizeof(T), kLoads = R / kVec;
    static_assert(R % kVec == 0, "a run is whole 16-byte pieces");
    if (cnt == R && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            const uint4 w = reinterpret_cast<const uint4*>(p)[i];
            T e[kVec];
            __builtin_memcpy(e, &w, 16);
#pragma unroll
            for (int j = 0; j < kVec; ++j) v[i * kVec + j] = (double)e[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = j < cnt ? (double)p[j] : 0.0;
    }
}

// q[0..cnt) = s[0..cnt) converted: 16-byte stores where the run is whole and aligned
template <class T, int R>
__device__ __forceinline__ void smooth_store_run(T* q, const int cnt, const double (&s)[R]) {
    constexpr int kVec = 16 / (int)sizeof(T), kStores = R / kVec;
    if (cnt == R && ((uintptr_t)q & 15u) == 0) {
#pragma unroll
        for (int i = 0; i < kStores; ++i) {
            T e[kVec];
#pragma unroll
            for (int j = 0; j < kVec; ++j) e[j] = smooth_convert(s[i * kVec + j], T());
            uint4 w;
            __builtin_memcpy(&w, e, 16);
            reinterpret_cast<uint4*>(q)[i] = w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (j < cnt) q[j] = smooth_convert(s[j], T());
    }
}

// ------------------------------------------------------------------------------------------------------------------ x pass
// grid ceil(rows / 4) * segs blocks, rows = D * H, segs = ceil(W / (64 * R)); block b is row block b / segs, segment b % segs
template <class Tin, class Tout, int R>
__global__ __launch_bounds__(256) void smooth_x_kernel(const Tin* __restrict__ in, Tout* __restrict__ out, const int rows, const int W,
                                                       const FastDiv div_segs, const double* __restrict__ w, const int r, const int border) {
    RPNET_PASS_PRIORITY();
    constexpr int TX = 64 * R;
    static_assert(R * (int)sizeof(Tin) == kSmoothRunBytes && smooth_pad(TX + 2 * RPNET_SMOOTH_MAX_RADIUS) < kSmoothPitch, "run and pitch");
    __shared__ double sw[kSmoothMaxTaps];
    __shared__ double tile[kSmoothXRows][kSmoothPitch];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int taps = 2 * r + 1;
    for (int i = t; i < taps; i += 256) sw[i] = w[i];
    unsigned rb;
    const int x0 = (int)div_segs.divmod(blockIdx.x, rb) * TX;
    const int row = (int)rb * kSmoothXRows + wv;
    const Tin* p = in + (size_t)min(row, rows - 1) * W;
    double* my = tile[wv];

    // the run of the lane, then the halo: position e of the staged row is x = x0 - r + e
    const int xr = x0 + lane * R;
    double v[R];
    if (xr + R <= W) {
        smooth_load_run<Tin, R>(p + xr, R, v);
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = (double)p[smooth_fold(xr + j, W, border)];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) my[smooth_pad(r + lane * R + j)] = v[j];
    for (int h = lane; h < 2 * r; h += 64) {
        const int e = h < r ? h : h + TX;
        my[smooth_pad(e)] = (double)p[smooth_fold(x0 - r + e, W, border)];
    }
    __syncthreads();

    // output j of the lane is position r + lane * R + j: its tap k + r = kk stands at position lane * R + j + kk
    double s[R], wr[R];
#pragma unroll
    for (int j = 0; j < R; ++j) s[j] = wr[j] = 0.0;
    const int steps = R + 2 * r;
    for (int i = 0; i < steps; ++i) {
#pragma unroll
        for (int j = R - 1; j > 0; --j) wr[j] = wr[j - 1];
        wr[0] = sw[min(i, 2 * r)];
        const double a = my[smooth_pad(lane * R + i)];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int kk = i - j;
            if (kk >= 0 && kk <= 2 * r) s[j] = __dadd_rn(s[j], __dmul_rn(wr[j], a));
        }
    }
    const int cnt = min(R, W - xr);
    if (row < rows && cnt > 0) smooth_store_run<Tout, R>(out + (size_t)row * W + xr, cnt, s);
}

// ----------------------------------------------------------------------------------------------------------- y and z passes
// [outer][n][inner], the pass along n.  lanes over (outer, segment of kSeg outputs along n, run of R along inner), runs fastest:
// n_lanes = outer * ceil(n / kSeg) * lpr < 2^26
template <class Tin, class Tout, int R>
__global__ __launch_bounds__(256) void smooth_col_kernel(const Tin* __restrict__ in, Tout* __restrict__ out, const int n, const int inner,
                                                         const FastDiv div_lpr, const FastDiv div_segs, const unsigned n_lanes, const int iters,
                                                         const double* __restrict__ w, const int r, const int border) {
    RPNET_PASS_PRIORITY();
    constexpr int kSeg = kSmoothSegVoxels / R;
    __shared__ double sw[kSmoothMaxTaps];
    const int t = threadIdx.x;
    const int taps = 2 * r + 1;
    for (int i = t; i < taps; i += 256) sw[i] = w[i];
    __syncthreads();
    const int steps = kSeg + 2 * r;
    for (int it = 0; it < iters; ++it) {
        const unsigned lane = ((unsigned)blockIdx.x * iters + it) * 256u + t;
        if (lane >= n_lanes) continue;
        unsigned q, o;
        const int c0 = (int)div_lpr.divmod(lane, q) * R;
        const int i0 = (int)div_segs.divmod(q, o) * kSeg;
        const int cnt = min(R, inner - c0);
        const Tin* p = in + (size_t)o * n * inner + c0;
        double s[kSeg][R], wr[kSeg];
#pragma unroll
        for (int j = 0; j < kSeg; ++j) {
            wr[j] = 0.0;
#pragma unroll
            for (int x = 0; x < R; ++x) s[j][x] = 0.0;
        }
        for (int i = 0; i < steps; ++i) {
            int idx = i0 - r + i;
            if ((unsigned)idx >= (unsigned)n) idx = smooth_fold(idx, n, border);
            double v[R];
            smooth_load_run<Tin, R>(p + (size_t)idx * inner, cnt, v);
#pragma unroll
            for (int j = kSeg - 1; j > 0; --j) wr[j] = wr[j - 1];
            wr[0] = sw[min(i, 2 * r)];
#pragma unroll
            for (int j = 0; j < kSeg; ++j) {
                const int kk = i - j;
                if (kk >= 0 && kk <= 2 * r) {
#pragma unroll
                    for (int x = 0; x < R; ++x) s[j][x] = __dadd_rn(s[j][x], __dmul_rn(wr[j], v[x]));
                }
            }
        }
        Tout* d = out + ((size_t)o * n + i0) * inner + c0;
#pragma unroll
        for (int j = 0; j < kSeg; ++j)
            if (i0 + j < n) smooth_store_run<Tout, R>(d + (size_t)j * inner, cnt, s[j]);
    }
}

// all radii 0: out = in, 16 bytes per lane
__global__ __launch_bounds__(256) void smooth_copy_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const size_t n, const size_t n_lanes,
                                                          const int iters) {
    RPNET_PASS_PRIORITY();
    for (int it = 0; it < iters; ++it) {
        const size_t lane = ((size_t)blockIdx.x * iters + it) * 256u + threadIdx.x;
        if (lane >= n_lanes) continue;
        const size_t base = lane * 16u;
        const int cnt = (int)std::min<size_t>((size_t)16, n - base);
        if (cnt == 16 && (((uintptr_t)(in + base) | (uintptr_t)(out + base)) & 15u) == 0) {
            *reinterpret_cast<uint4*>(out + base) = *reinterpret_cast<const uint4*>(in + base);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < cnt) out[base + j] = in[base + j];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
static inline bool smooth_radius_ok(int r) { return r >= 0 && r <= RPNET_SMOOTH_MAX_RADIUS; }
static inline size_t smooth_buffer_bytes(int D, int H, int W) { return 16 * (((size_t)D * H * W + 1) / 2); }
static inline size_t smooth_need(int D, int H, int W, int rz, int ry, int rx) {
    const int passes = (rz != 0) + (ry != 0) + (rx != 0);
    return kCcHeadBytes + smooth_buffer_bytes(D, H, W) * (size_t)std::min(2, std::max(0, passes - 1));
}
static inline bool smooth_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

template <class Tin, class Tout, int R>
static void smooth_x(const void* in, void* out, int rows, int W, const double* w, int r, int border, hipStream_t st) {
    const int segs = cdiv(W, 64 * R);
    hipLaunchKernelGGL((smooth_x_kernel<Tin, Tout, R>), dim3((unsigned)cdiv(rows, kSmoothXRows) * segs), dim3(256), 0, st, static_cast<const Tin*>(in),
                       static_cast<Tout*>(out), rows, W, FastDiv((unsigned)segs), w, r, border);
}

template <class Tin, class Tout, int R>
static void smooth_col(const void* in, void* out, int outer, int n, int inner, const double* w, int r, int border, hipStream_t st) {
    const int lpr = cdiv(inner, R), segs = cdiv(n, kSmoothSegVoxels / R);
    const size_t n_lanes = (size_t)outer * segs * lpr;                          // <= 2^30 / 32 + the ragged ends
    const int blocks = cc_sweep_blocks(n_lanes), iters = cc_sweep_iters(n_lanes, blocks);
    hipLaunchKernelGGL((smooth_col_kernel<Tin, Tout, R>), dim3(blocks), dim3(256), 0, st, static_cast<const Tin*>(in), static_cast<Tout*>(out), n, inner,
                       FastDiv((unsigned)lpr), FastDiv((unsigned)segs), (unsigned)n_lanes, iters, w, r, border);
}

// the passes of a call for a volume of kind T: the first reads T, the last writes T, float64 between them
template <class T>
static void smooth_passes(const void* in, void* out, int D, int H, int W, const double* wz, int rz, const double* wy, int ry, const double* wx, int rx,
                          int border, void* workspace, hipStream_t st) {
    constexpr int R = kSmoothRunBytes / (int)sizeof(T);
    const int passes = (rz != 0) + (ry != 0) + (rx != 0);
    char* ws = static_cast<char*>(workspace) + kCcHeadBytes;
    void* buf[2] = {ws, ws + smooth_buffer_bytes(D, H, W)};
    const void* src = in;
    bool wide = false;                              // is src float64
    int done = 0;
    if (rx) {
        const bool last = ++done == passes;
        void* dst = last ? out : buf[0];
        if (last) smooth_x<T, T, R>(src, dst, D * H, W, wx, rx, border, st);
        else smooth_x<T, double, R>(src, dst, D * H, W, wx, rx, border, st);
        src = dst;
        wide = true;
    }
    for (int axis = 1; axis >= 0; --axis) {         // y, then z
        const int r = axis ? ry : rz;
        if (!r) continue;
        const bool last = ++done == passes;
        void* dst = last ? out : (src == buf[0] ? buf[1] : buf[0]);
        const double* w = axis ? wy : wz;
        const int outer = axis ? D : 1, n = axis ? H : D, inner = axis ? W : H * W;
        if (wide && last) smooth_col<double, T, R>(src, dst, outer, n, inner, w, r, border, st);
        else if (wide) smooth_col<double, double, R>(src, dst, outer, n, inner, w, r, border, st);
        else if (last) smooth_col<T, T, R>(src, dst, outer, n, inner, w, r, border, st);
        else smooth_col<T, double, R>(src, dst, outer, n, inner, w, r, border, st);
        src = dst;
        wide = true;
    }
}

}  // namespace rpnet

extern "C" int rpnet_smooth_abi_version(void) { return RPNET_SMOOTH_ABI_VERSION; }

extern "C" size_t rpnet_smooth_workspace_bytes(int D, int H, int W, int rz, int ry, int rx) {
    using namespace rpnet;
    if (!cc_dims_ok(D, H, W) || !smooth_radius_ok(rz) || !smooth_radius_ok(ry) || !smooth_radius_ok(rx)) {
        set_error("smooth: D=%d H=%d W=%d, radii z=%d y=%d x=%d (every extent 1..%d, every radius 0..%d)", D, H, W, rz, ry, rx, RPNET_CC_MAX_DIM,
                  RPNET_SMOOTH_MAX_RADIUS);
        return 0;
    }
    return smooth_need(D, H, W, rz, ry, rx);
}

extern "C" int rpnet_smooth_image(const void* in, int kind, int D, int H, int W, void* out, const double* wz, int rz, const double* wy, int ry,
                                  const double* wx, int rx, int border, void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    const char* fn = "smooth_image";
    RPNET_REQUIRE(in && out && workspace, RPNET_ERR_ARG, "%s: null pointer", fn);
    RPNET_REQUIRE(kind == RPNET_PREP_F32 || kind == RPNET_PREP_I16, RPNET_ERR_ARG, "%s: element kind %d (0 float32, 1 int16)", fn, kind);
    RPNET_REQUIRE(border == RPNET_SMOOTH_REFLECT || border == RPNET_SMOOTH_NEAREST, RPNET_ERR_ARG, "%s: border %d (0 reflect, 1 nearest)", fn, border);
    RPNET_REQUIRE(cc_dims_ok(D, H, W), RPNET_ERR_SHAPE, "%s: D=%d H=%d W=%d (every extent 1..%d)", fn, D, H, W, RPNET_CC_MAX_DIM);
    RPNET_REQUIRE(smooth_radius_ok(rz) && smooth_radius_ok(ry) && smooth_radius_ok(rx), RPNET_ERR_ARG, "%s: radii z=%d y=%d x=%d (every radius 0..%d)", fn,
                  rz, ry, rx, RPNET_SMOOTH_MAX_RADIUS);
    RPNET_REQUIRE((wz != nullptr) == (rz != 0) && (wy != nullptr) == (ry != 0) && (wx != nullptr) == (rx != 0), RPNET_ERR_ARG,
                  "%s: a weight table is null exactly when its radius is 0 (radii z=%d y=%d x=%d)", fn, rz, ry, rx);
    const size_t need = smooth_need(D, H, W, rz, ry, rx);
    RPNET_REQUIRE(workspace_bytes >= need, RPNET_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    const size_t es = kind == RPNET_PREP_F32 ? 4 : 2, bytes = (size_t)D * H * W * es;
    RPNET_REQUIRE(((uintptr_t)in % es) == 0 && ((uintptr_t)out % es) == 0 && ((uintptr_t)workspace % 16) == 0, RPNET_ERR_ARG,
                  "%s: the volumes must be aligned to their element and the workspace to 16 bytes", fn);
    RPNET_REQUIRE(((uintptr_t)wz % 8) == 0 && ((uintptr_t)wy % 8) == 0 && ((uintptr_t)wx % 8) == 0, RPNET_ERR_ARG,
                  "%s: the weight tables must be aligned to 8 bytes", fn);
    RPNET_REQUIRE(smooth_disjoint(in, bytes, out, bytes), RPNET_ERR_ARG, "%s: out overlaps in", fn);
    RPNET_REQUIRE(smooth_disjoint(in, bytes, workspace, need) && smooth_disjoint(out, bytes, workspace, need), RPNET_ERR_ARG,
                  "%s: the workspace overlaps a volume", fn);
    hipStream_t st = (hipStream_t)stream;
    if (!rz && !ry && !rx) {
        const size_t n_lanes = (bytes + 15) / 16;
        const int blocks = cc_sweep_blocks(n_lanes);
        hipLaunchKernelGGL(smooth_copy_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), bytes, n_lanes,
                           cc_sweep_iters(n_lanes, blocks));
    } else if (kind == RPNET_PREP_F32) {
        smooth_passes<float>(in, out, D, H, W, wz, rz, wy, ry, wx, rx, border, workspace, st);
    } else {
        smooth_passes<int16_t>(in, out, D, H, W, wz, rz, wy, ry, wx, rx, border, workspace, st);
    }
    return check_launch(fn);
}
