// The evaluation item of a data-set run, assembled on the device (rpnet_amd/dataset_eval.py; the host restatement is
// FewshotSliceReader's eval branch, rpnet_amd/utils/volume_reader.py, after dataset/few_shot_reader.py:523-546), and the two image
// similarity figures the driver prints per volume (test_rpnet.py:229-230).
//
//   eval_item_gather_kernel   ONE launch for the whole item: query slice s is paired with support slice support_slice[s] (the k-block
//                             table the host builds); writes the support image / label and the query image / label in the form the
//                             model takes, and the two [0,1] planes (x + 1) / 2 that feed the registration.  Four planes in, six out,
//                             nothing else: HBM-bound, 16-byte accesses along W, the W % 4 columns of a row one by one.
//   ncc_sums_kernel           pass 1 of NCC: the sums of the three tensors, fp64, one partial row per block
//   ncc_centred_kernel        pass 2: every block forms the three means from ALL partial rows in the same fixed order (so that all
//                             blocks hold the same bits), then its share of sum f m, sum f^2, sum m^2 for both pairs
//   ncc_finish_kernel         one block adds the partial rows in a fixed order and writes the two figures
// No atomics anywhere: the order of every sum is a function of the element count alone, two runs give the same bits.  The centred
// two-pass form is the reference's own (net/registration.py:16-20): a constant image gives f == 0 exactly (the fp64 sum of n equal
// fp32 values is exact for n < 2^29), not the cancellation residue of the raw-moment form, which would sit beside the 1e-10 term.
#include "common.h"
#include "rpnet_eval_abi.h"

namespace rpnet {

// a 16-byte vector that may sit on a 4-byte boundary (rows of a plane whose W is no multiple of 4)
typedef f32x4 f32x4_u __attribute__((aligned(4)));

// (x + 1) / 2 as the host forms it: one fp32 add, one fp32 multiply by 0.5 (no contraction into an fma)
__device__ __forceinline__ float unit_map(const float x) { return __fmul_rn(__fadd_rn(x, 1.f), 0.5f); }

template <typename V>
__device__ __forceinline__ void gather_quad(const float* __restrict__ si, const float* __restrict__ sm, const float* __restrict__ qi,
                                            const float* __restrict__ qm, float* __restrict__ o_si, float* __restrict__ o_sm,
                                            float* __restrict__ o_qi, float* __restrict__ o_qm, float* __restrict__ o_sr,
                                            float* __restrict__ o_qr) {
    const f32x4 a = *reinterpret_cast<const V*>(si), b = *reinterpret_cast<const V*>(sm);
    const f32x4 c = *reinterpret_cast<const V*>(qi), d = *reinterpret_cast<const V*>(qm);
    f32x4 ar, cr;
#pragma unroll
    for (int j = 0; j < 4; ++j) { ar[j] = unit_map(a[j]); cr[j] = unit_map(c[j]); }
    *reinterpret_cast<V*>(o_si) = a;
    *reinterpret_cast<V*>(o_sm) = b;
    *reinterpret_cast<V*>(o_qi) = c;
    *reinterpret_cast<V*>(o_qm) = d;
    *reinterpret_cast<V*>(o_sr) = ar;
    *reinterpret_cast<V*>(o_qr) = cr;
}

// grid (cdiv(H * Q, 256), S), Q = cdiv(W, 4) quads per row; a thread owns one quad (or the W % 4 tail) of one row of one slice.
// ALIGNED: W % 4 == 0 and every base pointer on a 16-byte boundary.  A table entry outside [0, Ds) is the caller's error (the Python
// side refuses it before the upload); it is clamped here so that the launch never reads outside the volume.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void eval_item_gather_kernel(const float* __restrict__ s_img, const float* __restrict__ s_msk,
                                                               const float* __restrict__ q_img, const float* __restrict__ q_msk,
                                                               const int32_t* __restrict__ support_slice, float* __restrict__ sup_img,
                                                               float* __restrict__ sup_lab, float* __restrict__ qry_img,
                                                               float* __restrict__ qry_lab, float* __restrict__ sup_reg,
                                                               float* __restrict__ qry_reg, const int Ds, const int H, const int W,
                                                               const unsigned units, const FastDiv div_q) {
    RPNET_PASS_PRIORITY();
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const int s = blockIdx.y;
    const int z = min(max(support_slice[s], 0), Ds - 1);
    unsigned y;
    const unsigned x = div_q.divmod(u, y) * 4u;
    const size_t HW = (size_t)H * W, in_row = (size_t)y * W + x;
    const size_t so = (size_t)z * HW + in_row, qo = (size_t)s * HW + in_row;
    if (x + 4u <= (unsigned)W) {
        if (ALIGNED)
            gather_quad<f32x4>(s_img + so, s_msk + so, q_img + qo, q_msk + qo, sup_img + qo, sup_lab + qo, qry_img + qo, qry_lab + qo,
                               sup_reg + qo, qry_reg + qo);
        else
            gather_quad<f32x4_u>(s_img + so, s_msk + so, q_img + qo, q_msk + qo, sup_img + qo, sup_lab + qo, qry_img + qo, qry_lab + qo,
                                 sup_reg + qo, qry_reg + qo);
        return;
    }
    for (unsigned j = 0; x + j < (unsigned)W; ++j) {          // the W % 4 columns at the end of the row
        const float a = s_img[so + j], c = q_img[qo + j];
        sup_img[qo + j] = a;
        sup_lab[qo + j] = s_msk[so + j];
        qry_img[qo + j] = c;
        qry_lab[qo + j] = q_msk[qo + j];
        sup_reg[qo + j] = unit_map(a);
        qry_reg[qo + j] = unit_map(c);
    }
}

// ------------------------------------------------------------------------------------------------------------------ NCC
constexpr int kNccMaxBlocks = 1024;          // partial rows per pass
constexpr int kNccRow = 8;                   // doubles per partial row (pass 1 uses 3, pass 2 uses 5)
constexpr size_t kNccPerBlock = 4096;        // elements a block takes before another block is added

static int ncc_blocks(size_t n) {
    const size_t b = (n + kNccPerBlock - 1) / kNccPerBlock;
    return (int)(b < 1 ? 1 : b > (size_t)kNccMaxBlocks ? (size_t)kNccMaxBlocks : b);
}

// the three sums of pass 1 from all partial rows, the same order in every block that asks: thread t takes rows t, t + 256, ...,
// then the block sum.  Valid in every thread.
__device__ __forceinline__ void ncc_totals(const double* __restrict__ part, const int rows, double* smem4, double (&tot)[3]) {
    double a[3] = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] += part[(size_t)r * kNccRow + j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) tot[j] = block_sum256(a[j], smem4);
}

// part1 [gridDim.x][kNccRow]: {sum q, sum w, sum a}.  The first nvec * 4 elements as 16-byte loads (nvec == 0 when a pointer is not
// 16-byte aligned), the rest one by one.
__global__ __launch_bounds__(256) void ncc_sums_kernel(const float* __restrict__ q, const float* __restrict__ w, const float* __restrict__ a,
                                                       double* __restrict__ part1, const size_t n, const size_t nvec) {
    RPNET_PASS_PRIORITY();
    __shared__ double smem4[4];
    double s[3] = {0.0, 0.0, 0.0};
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t i = first; i < nvec; i += stride) {
        const f32x4 vq = reinterpret_cast<const f32x4*>(q)[i], vw = reinterpret_cast<const f32x4*>(w)[i];
        const f32x4 va = reinterpret_cast<const f32x4*>(a)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[0] += (double)vq[j]; s[1] += (double)vw[j]; s[2] += (double)va[j]; }
    }
    for (size_t i = nvec * 4 + first; i < n; i += stride) { s[0] += (double)q[i]; s[1] += (double)w[i]; s[2] += (double)a[i]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double t = block_sum256(s[j], smem4);
        if (threadIdx.x == 0) part1[(size_t)blockIdx.x * kNccRow + j] = t;
    }
}

// part2 [gridDim.x][kNccRow]: {sum m^2, sum fw^2, sum fw m, sum fa^2, sum fa m}, m = q - mean q, fw = w - mean w, fa = a - mean a
__global__ __launch_bounds__(256) void ncc_centred_kernel(const float* __restrict__ q, const float* __restrict__ w,
                                                          const float* __restrict__ a, const double* __restrict__ part1,
                                                          double* __restrict__ part2, const size_t n, const size_t nvec) {
    RPNET_PASS_PRIORITY();
    __shared__ double smem4[4];
    double tot[3];
    ncc_totals(part1, gridDim.x, smem4, tot);
    const double mq = tot[0] / (double)n, mw = tot[1] / (double)n, ma = tot[2] / (double)n;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    auto take = [&](const float xq, const float xw, const float xa) {
        const double m = (double)xq - mq, fw = (double)xw - mw, fa = (double)xa - ma;
        s[0] += m * m;
        s[1] += fw * fw;
        s[2] += fw * m;
        s[3] += fa * fa;
        s[4] += fa * m;
    };
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t i = first; i < nvec; i += stride) {
        const f32x4 vq = reinterpret_cast<const f32x4*>(q)[i], vw = reinterpret_cast<const f32x4*>(w)[i];
        const f32x4 va = reinterpret_cast<const f32x4*>(a)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) take(vq[j], vw[j], va[j]);
    }
    for (size_t i = nvec * 4 + first; i < n; i += stride) take(q[i], w[i], a[i]);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double t = block_sum256(s[j], smem4);
        if (threadIdx.x == 0) part2[(size_t)blockIdx.x * kNccRow + j] = t;
    }
}

// out[0] = NCC(q, w), out[1] = NCC(q, a): -sum(f m) / sqrt(sum f^2 sum m^2 + 1e-10).  One block.
__global__ __launch_bounds__(256) void ncc_finish_kernel(const double* __restrict__ part2, const int rows, double* __restrict__ out) {
    __shared__ double smem4[4];
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, tot[5];
    for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int j = 0; j < 5; ++j) s[j] += part2[(size_t)r * kNccRow + j];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) tot[j] = block_sum256(s[j], smem4);
    if (threadIdx.x == 0) {
        out[0] = -1.0 * tot[2] / sqrt(tot[1] * tot[0] + 1e-10);
        out[1] = -1.0 * tot[4] / sqrt(tot[3] * tot[0] + 1e-10);
    }
}

}  // namespace rpnet

extern "C" int rpnet_eval_abi_version(void) { return RPNET_EVAL_ABI_VERSION; }

extern "C" int rpnet_eval_item_gather(const float* s_img, const float* s_msk, const float* q_img, const float* q_msk,
                                      const int32_t* support_slice, float* sup_img, float* sup_lab, float* qry_img, float* qry_lab,
                                      float* sup_reg, float* qry_reg, int Ds, int S, int H, int W, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(Ds >= 1 && S >= 1 && H >= 1 && W >= 1, RPNET_ERR_SHAPE,
                  "eval_item_gather: support depth %d, S=%d H=%d W=%d (an empty volume or item is refused)", Ds, S, H, W);
    RPNET_REQUIRE(s_img && s_msk && q_img && q_msk && support_slice && sup_img && sup_lab && qry_img && qry_lab && sup_reg && qry_reg,
                  RPNET_ERR_ARG, "eval_item_gather: null pointer");
    RPNET_REQUIRE(S <= 65535, RPNET_ERR_SHAPE, "eval_item_gather: %d slices (at most 65535 per call)", S);
    const size_t HW = (size_t)H * W;
    RPNET_REQUIRE((size_t)S * HW < kIndex32 && (size_t)Ds * HW < kIndex32, RPNET_ERR_SHAPE,
                  "eval_item_gather: S*H*W = %zu / Ds*H*W = %zu does not fit the 32-bit index arithmetic", (size_t)S * HW, (size_t)Ds * HW);
    const float* outs[6] = {sup_img, sup_lab, qry_img, qry_lab, sup_reg, qry_reg};
    const float* ins[4] = {s_img, s_msk, q_img, q_msk};
    bool aligned = W % 4 == 0;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 4; ++j) RPNET_REQUIRE(outs[i] != ins[j], RPNET_ERR_ARG, "eval_item_gather: a gather cannot run in place");
        for (int j = 0; j < i; ++j) RPNET_REQUIRE(outs[i] != outs[j], RPNET_ERR_ARG, "eval_item_gather: two outputs share their memory");
        RPNET_REQUIRE(((uintptr_t)outs[i] % 4) == 0, RPNET_ERR_ARG, "eval_item_gather: output %d is not 4-byte aligned", i);
        aligned = aligned && ((uintptr_t)outs[i] % 16) == 0;
    }
    for (int j = 0; j < 4; ++j) {
        RPNET_REQUIRE(((uintptr_t)ins[j] % 4) == 0, RPNET_ERR_ARG, "eval_item_gather: input %d is not 4-byte aligned", j);
        aligned = aligned && ((uintptr_t)ins[j] % 16) == 0;
    }
    const unsigned Q = (unsigned)((W + 3) / 4), units = (unsigned)H * Q;
    const dim3 grid(cdiv((long)units, 256), S);
    if (aligned)
        hipLaunchKernelGGL(eval_item_gather_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, s_img, s_msk, q_img, q_msk, support_slice,
                           sup_img, sup_lab, qry_img, qry_lab, sup_reg, qry_reg, Ds, H, W, units, FastDiv(Q));
    else
        hipLaunchKernelGGL(eval_item_gather_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, s_img, s_msk, q_img, q_msk, support_slice,
                           sup_img, sup_lab, qry_img, qry_lab, sup_reg, qry_reg, Ds, H, W, units, FastDiv(Q));
    return check_launch("eval_item_gather");
}

extern "C" size_t rpnet_ncc_pairs_workspace_bytes(size_t n) {
    using namespace rpnet;
    return 2 * (size_t)ncc_blocks(n) * kNccRow * sizeof(double);
}

extern "C" int rpnet_ncc_pairs(const float* query, const float* warped, const float* affine, size_t n, double* table, int row, int n_rows,
                               void* workspace, size_t workspace_bytes, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(n >= 1, RPNET_ERR_SHAPE, "ncc_pairs: empty tensors");
    RPNET_REQUIRE(query && warped && affine && table && workspace, RPNET_ERR_ARG, "ncc_pairs: null pointer");
    RPNET_REQUIRE(n < ((size_t)1 << 29), RPNET_ERR_SHAPE, "ncc_pairs: %zu elements (fewer than 2^29: the sum of a constant image stays exact)", n);
    RPNET_REQUIRE(row >= 0 && row < n_rows, RPNET_ERR_ARG, "ncc_pairs: row %d of a table of %d rows", row, n_rows);
    RPNET_REQUIRE(((uintptr_t)query % 4) == 0 && ((uintptr_t)warped % 4) == 0 && ((uintptr_t)affine % 4) == 0, RPNET_ERR_ARG,
                  "ncc_pairs: the images must be 4-byte aligned");
    RPNET_REQUIRE(((uintptr_t)table % 8) == 0 && ((uintptr_t)workspace % 8) == 0, RPNET_ERR_ARG, "ncc_pairs: table and workspace must be 8-byte aligned");
    RPNET_REQUIRE(workspace_bytes >= rpnet_ncc_pairs_workspace_bytes(n), RPNET_ERR_WORKSPACE, "ncc_pairs: workspace of %zu bytes, %zu needed",
                  workspace_bytes, rpnet_ncc_pairs_workspace_bytes(n));
    const int blocks = ncc_blocks(n);
    const bool vec = ((uintptr_t)query % 16) == 0 && ((uintptr_t)warped % 16) == 0 && ((uintptr_t)affine % 16) == 0;
    const size_t nvec = vec ? n / 4 : 0;
    double* part1 = (double*)workspace;
    double* part2 = part1 + (size_t)blocks * kNccRow;
    hipLaunchKernelGGL(ncc_sums_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, query, warped, affine, part1, n, nvec);
    hipLaunchKernelGGL(ncc_centred_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, query, warped, affine, (const double*)part1, part2, n,
                       nvec);
    hipLaunchKernelGGL(ncc_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part2, blocks, table + (size_t)row * 2);
    return check_launch("ncc_pairs");
}
