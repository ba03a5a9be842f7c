// Adam over the flat gradient bucket (rpnet_amd/optim.py: FusedAdam; include/rpnet_optim_abi.h).
//
//   plan (host)            the chunk table: every parameter cut into runs of at most RPNET_ADAM_CHUNK elements, each with the parameter
//                          pointer advanced to the run, its start in the flat buffers and whether it may go 16 bytes at a time
//   adam_advance_kernel    one wave: step += 1, the bias corrections in fp64 (torch.optim.Adam forms them in Python floats), then the
//                          seven scalars of the update rounded to fp32 once
//   adam_update_kernel     grid-stride over the table, a block per chunk: reads g, p, m, v and writes p, m, v — 28 bytes per element,
//                          the one pass the update needs.  HBM-bound; 16-byte accesses wherever the table allows them.
// The guarded step (include/rpnet_guard_abi.h) puts two launches in front and takes the GUARDED form of the update:
//   grad_sumsq_kernel            the same walk over the table, reading g alone: one fp64 sum of squares per chunk, in a fixed order
//   adam_advance_guarded_kernel  one block: adds the partials, forms norm, clip coefficient and the skip decision, and advances
//                                unless the step is skipped
// The update's arithmetic is spelled out with the rounding intrinsics, so that the compiler neither fuses nor splits an operation: it is
// the sequence torch's CPU Adam executes (lerp and addcmul as fused multiply-adds, addcdiv as a product, a division and a sum), and its
// rounding error against an fp64 Adam is therefore torch's own.
#include <math.h>

#include "common.h"
#include "rpnet_guard_abi.h"
#include "rpnet_optim_abi.h"

namespace rpnet {

static_assert(sizeof(rpnet_adam_chunk) == 24, "rpnet_adam_chunk is 24 bytes");
static_assert(sizeof(rpnet_adam_hyper) == 96, "rpnet_adam_hyper is 96 bytes");
static_assert(RPNET_ADAM_CHUNK >= 1 && RPNET_ADAM_CHUNK <= (1 << 30), "a chunk's count is an int32");

constexpr int kAdamMaxBlocks = 2048;
constexpr int64_t kAdamMaxTotal = (int64_t)1 << 40;

// one lane: the scalars go out as ordinary stores from a vector lane
__device__ __forceinline__ void adam_advance(rpnet_adam_hyper* __restrict__ h) {
    const int64_t step = h->step + 1;
    h->step = step;
    const double bc1 = 1.0 - pow(h->beta1, (double)step);
    const double bc2 = 1.0 - pow(h->beta2, (double)step);
    h->step_size = (float)(h->lr / bc1);
    h->bc2_sqrt = (float)sqrt(bc2);
    h->eps_f = (float)h->eps;
    h->weight_decay_f = (float)h->weight_decay;
    h->grad_scale_f = (float)h->grad_scale;
    h->beta1_f = (float)h->beta1;
    h->beta2_f = (float)h->beta2;
    h->one_minus_beta1 = (float)(1.0 - h->beta1);
    h->one_minus_beta2 = (float)(1.0 - h->beta2);
}

__global__ __launch_bounds__(64) void adam_advance_kernel(rpnet_adam_hyper* __restrict__ h) {
    if (threadIdx.x != 0) return;
    adam_advance(h);
}

struct AdamScalars {
    float neg_step_size, bc2_sqrt, eps, weight_decay, grad_scale, beta2, omb1, omb2;
};

// GUARDED: the scaled gradient times the clip coefficient, the two products in torch's order (flat.mul_(scale), then
// clip_grad_norm_'s g.mul_(coef)); coef == 1.0f multiplies exactly
template <bool GUARDED>
__device__ __forceinline__ void adam_element(const AdamScalars& s, const float coef, const float g, float& p, float& m, float& v) {
    const float gs = __fmul_rn(s.grad_scale, g);
    const float gp = __fmaf_rn(s.weight_decay, p, GUARDED ? __fmul_rn(coef, gs) : gs);
    m = __fmaf_rn(s.omb1, __fsub_rn(gp, m), m);
    v = __fmaf_rn(__fmul_rn(s.omb2, gp), gp, __fmul_rn(v, s.beta2));
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), s.bc2_sqrt), s.eps);
    p = __fadd_rn(p, __fdiv_rn(__fmul_rn(s.neg_step_size, m), denom));
}

// VEC: g, m and v are 16-byte aligned at their base, so a chunk whose table entry says vec16 takes 16-byte accesses
// GUARDED: `guard` holds the skip decision and the clip coefficient of this step (adam_advance_guarded_kernel); a skipped step
// writes nothing.  Without GUARDED the pointer is null and never read.
template <bool VEC, bool GUARDED>
__global__ __launch_bounds__(256) void adam_update_kernel(const rpnet_adam_chunk* __restrict__ table, const long n_chunks,
                                                          const float* __restrict__ grad, float* __restrict__ m_flat,
                                                          float* __restrict__ v_flat, const rpnet_adam_hyper* __restrict__ h,
                                                          const rpnet_grad_guard* __restrict__ guard) {
    float coef = 1.0f;
    if constexpr (GUARDED) {
        if (guard->skip) return;
        coef = guard->coef_f;
    }
    AdamScalars s;
    s.neg_step_size = -h->step_size;
    s.bc2_sqrt = h->bc2_sqrt;
    s.eps = h->eps_f;
    s.weight_decay = h->weight_decay_f;
    s.grad_scale = h->grad_scale_f;
    s.beta2 = h->beta2_f;
    s.omb1 = h->one_minus_beta1;
    s.omb2 = h->one_minus_beta2;
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const rpnet_adam_chunk e = table[c];
        float* __restrict__ p = e.param;
        const float* __restrict__ g = grad + e.flat_start;
        float* __restrict__ m = m_flat + e.flat_start;
        float* __restrict__ v = v_flat + e.flat_start;
        const int count = e.count;
        const int quads = (VEC && e.vec16) ? count >> 2 : 0;
        for (int i = threadIdx.x; i < quads; i += 256) {
            const f32x4 vg = reinterpret_cast<const f32x4*>(g)[i];
            f32x4 vp = reinterpret_cast<f32x4*>(p)[i], vm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = vp[j], mj = vm[j], vj = vv[j];
                adam_element<GUARDED>(s, coef, vg[j], pj, mj, vj);
                vp[j] = pj;
                vm[j] = mj;
                vv[j] = vj;
            }
            reinterpret_cast<f32x4*>(p)[i] = vp;
            reinterpret_cast<f32x4*>(m)[i] = vm;
            reinterpret_cast<f32x4*>(v)[i] = vv;
        }
        for (int i = quads * 4 + threadIdx.x; i < count; i += 256) {
            float pj = p[i], mj = m[i], vj = v[i];
            adam_element<GUARDED>(s, coef, g[i], pj, mj, vj);
            p[i] = pj;
            m[i] = mj;
            v[i] = vj;
        }
    }
}

// One fp64 sum of squares per chunk of the table, the walk and the quad / tail split of adam_update_kernel.  A lane adds its squares
// in index order (at most 16 of a full chunk; the square of an fp32 value is exact in fp64, only the additions round), block_sum256
// adds the lanes of a wave and then the four waves in wave order: partials[c] depends on the chunk alone, not on the grid.
template <bool VEC>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const rpnet_adam_chunk* __restrict__ table, const long n_chunks,
                                                         const float* __restrict__ grad, double* __restrict__ partials) {
    __shared__ double smem4[4];
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const rpnet_adam_chunk e = table[c];
        const float* __restrict__ g = grad + e.flat_start;
        const int count = e.count;
        const int quads = (VEC && e.vec16) ? count >> 2 : 0;
        double acc = 0.0;
        for (int i = threadIdx.x; i < quads; i += 256) {
            const f32x4 vg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double x = (double)vg[j];
                acc += x * x;
            }
        }
        for (int i = quads * 4 + threadIdx.x; i < count; i += 256) {
            const double x = (double)g[i];
            acc += x * x;
        }
        const double total = block_sum256(acc, smem4);
        if (threadIdx.x == 0) partials[c] = total;
    }
}

// One block of 256.  Thread t adds partials[t], partials[t + 256], ... in that order, block_sum256 adds the 256 sums: a fixed order.
// Lane 0 then forms the norm, the coefficient and the skip decision, records them, and advances unless the step is skipped.
// h == nullptr (rpnet_grad_sumsq): no optimizer, so no grad_scale, no advance and no step counters.
__global__ __launch_bounds__(256) void adam_advance_guarded_kernel(const double* __restrict__ partials, const long n_chunks,
                                                                   rpnet_adam_hyper* __restrict__ h, rpnet_grad_guard* __restrict__ gd,
                                                                   double* __restrict__ history) {
    __shared__ double smem4[4];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n_chunks; i += 256) acc += partials[i];
    const double sumsq = block_sum256(acc, smem4);
    if (threadIdx.x != 0) return;
    const double norm = (h ? fabs(h->grad_scale) : 1.0) * sqrt(sumsq);
    const double c = gd->max_norm / (norm + 1e-6);
    const double coef = c > 1.0 ? 1.0 : c;            // torch.clamp(c, max=1): a NaN stays a NaN
    const bool skip = gd->skip_nonfinite != 0 && !isfinite(sumsq);
    gd->sumsq = sumsq;
    gd->norm = norm;
    gd->coef = coef;
    gd->skip = skip ? 1 : 0;
    const int64_t attempt = gd->attempt;
    const int64_t capacity = gd->history_capacity;
    if (history && capacity > 0) {
        double* row = history + RPNET_GUARD_HISTORY_ROW * (attempt % capacity);
        row[0] = norm;
        row[1] = coef;
        row[2] = skip ? 1.0 : 0.0;
    }
    gd->attempt = attempt + 1;
    if (!skip) gd->coef_f = (float)coef;
    if (!h) return;
    if (skip) {
        gd->skipped += 1;
        return;
    }
    if (coef < 1.0) gd->clipped += 1;
    adam_advance(h);
}

// chunks of n parameters, or -1 with the error string set
static int64_t adam_count_chunks(const int64_t* counts, int n) {
    if (!counts || n < 1) {
        set_error("adam_plan: %d parameters, counts %s", n, counts ? "given" : "null");
        return -1;
    }
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (counts[i] < 1) {
            set_error("adam_plan: parameter %d has %lld elements (at least 1)", i, (long long)counts[i]);
            return -1;
        }
        if (counts[i] >= kAdamMaxTotal) {
            set_error("adam_plan: parameter %d has %lld elements (the flat buffer holds fewer than 2^40)", i, (long long)counts[i]);
            return -1;
        }
        chunks += (counts[i] + RPNET_ADAM_CHUNK - 1) / RPNET_ADAM_CHUNK;
    }
    return chunks;
}

}  // namespace rpnet

extern "C" int rpnet_optim_abi_version(void) { return RPNET_OPTIM_ABI_VERSION; }

extern "C" size_t rpnet_adam_plan_bytes(const int64_t* counts, int n) {
    const int64_t chunks = rpnet::adam_count_chunks(counts, n);
    return chunks < 0 ? 0 : (size_t)chunks * sizeof(rpnet_adam_chunk);
}

extern "C" int rpnet_adam_plan(const void* const* params, const int64_t* counts, const int64_t* offsets, int n, void* table,
                               size_t table_bytes, int64_t* n_chunks) {
    using namespace rpnet;
    RPNET_REQUIRE(params && counts && offsets && table && n_chunks, RPNET_ERR_ARG, "adam_plan: null argument");
    RPNET_REQUIRE(n >= 1, RPNET_ERR_ARG, "adam_plan: %d parameters", n);
    const int64_t chunks = adam_count_chunks(counts, n);
    if (chunks < 0) return RPNET_ERR_SHAPE;
    int64_t end = 0;
    for (int i = 0; i < n; ++i) {
        RPNET_REQUIRE(params[i] != nullptr, RPNET_ERR_ARG, "adam_plan: parameter %d is a null pointer", i);
        RPNET_REQUIRE(((uintptr_t)params[i] % 4) == 0, RPNET_ERR_ARG, "adam_plan: parameter %d is not 4-byte aligned", i);
        RPNET_REQUIRE(offsets[i] >= end, RPNET_ERR_ARG,
                      "adam_plan: parameter %d starts at %lld in the flat buffer, the one before it ends at %lld (offsets ascend "
                      "and do not overlap)", i, (long long)offsets[i], (long long)end);
        RPNET_REQUIRE(offsets[i] < kAdamMaxTotal, RPNET_ERR_SHAPE, "adam_plan: parameter %d starts at %lld (fewer than 2^40 elements)", i,
                      (long long)offsets[i]);
        end = offsets[i] + counts[i];
        RPNET_REQUIRE(end < kAdamMaxTotal, RPNET_ERR_SHAPE, "adam_plan: the flat buffer ends at %lld (fewer than 2^40 elements)",
                      (long long)end);
    }
    RPNET_REQUIRE(table_bytes >= (size_t)chunks * sizeof(rpnet_adam_chunk), RPNET_ERR_WORKSPACE,
                  "adam_plan: table buffer of %zu bytes, %zu needed", table_bytes, (size_t)chunks * sizeof(rpnet_adam_chunk));
    rpnet_adam_chunk* out = (rpnet_adam_chunk*)table;
    int64_t k = 0;
    for (int i = 0; i < n; ++i) {
        for (int64_t done = 0; done < counts[i]; done += RPNET_ADAM_CHUNK, ++k) {
            const int64_t left = counts[i] - done;
            float* p = (float*)params[i] + done;
            out[k].param = p;
            out[k].flat_start = offsets[i] + done;
            out[k].count = (int32_t)(left < RPNET_ADAM_CHUNK ? left : RPNET_ADAM_CHUNK);
            out[k].vec16 = (out[k].flat_start % 4 == 0 && ((uintptr_t)p % 16) == 0) ? 1 : 0;
        }
    }
    *n_chunks = k;
    return RPNET_OK;
}

extern "C" int rpnet_adam_step(const struct rpnet_adam_chunk* table, int64_t n_chunks, const float* grad, float* m, float* v,
                               struct rpnet_adam_hyper* hyper, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(table && grad && m && v && hyper, RPNET_ERR_ARG, "adam_step: null pointer");
    RPNET_REQUIRE(n_chunks >= 1 && n_chunks < kAdamMaxTotal, RPNET_ERR_SHAPE, "adam_step: %lld chunks", (long long)n_chunks);
    RPNET_REQUIRE(((uintptr_t)table % 8) == 0 && ((uintptr_t)hyper % 8) == 0, RPNET_ERR_ARG,
                  "adam_step: the table and the hyper-parameter block must be 8-byte aligned");
    RPNET_REQUIRE(((uintptr_t)grad % 4) == 0 && ((uintptr_t)m % 4) == 0 && ((uintptr_t)v % 4) == 0, RPNET_ERR_ARG,
                  "adam_step: grad, m and v must be 4-byte aligned");
    RPNET_REQUIRE(grad != m && grad != v && m != v, RPNET_ERR_ARG, "adam_step: grad, m and v are three buffers");
    const bool vec = ((uintptr_t)grad % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0;
    const int blocks = (int)(n_chunks < kAdamMaxBlocks ? n_chunks : kAdamMaxBlocks);
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper);
    const rpnet_grad_guard* none = nullptr;
    if (vec)
        hipLaunchKernelGGL((adam_update_kernel<true, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, table, (long)n_chunks,
                           grad, m, v, (const rpnet_adam_hyper*)hyper, none);
    else
        hipLaunchKernelGGL((adam_update_kernel<false, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, table, (long)n_chunks,
                           grad, m, v, (const rpnet_adam_hyper*)hyper, none);
    return check_launch("adam_step");
}

// ------------------------------------------------------------------------------------------------ the guard (include/rpnet_guard_abi.h)
extern "C" int rpnet_guard_abi_version(void) { return RPNET_GUARD_ABI_VERSION; }

extern "C" int rpnet_grad_guard_init(struct rpnet_grad_guard* host_block, double max_norm, int skip_nonfinite,
                                     int64_t history_capacity) {
    using namespace rpnet;
    RPNET_REQUIRE(host_block, RPNET_ERR_ARG, "grad_guard_init: null block");
    RPNET_REQUIRE(max_norm > 0.0, RPNET_ERR_ARG, "grad_guard_init: max_norm %g (greater than 0; +inf: no clipping)", max_norm);
    RPNET_REQUIRE(history_capacity >= 0, RPNET_ERR_ARG, "grad_guard_init: history_capacity %lld (0: no ring)",
                  (long long)history_capacity);
    *host_block = rpnet_grad_guard{};
    host_block->max_norm = max_norm;
    host_block->skip_nonfinite = skip_nonfinite ? 1 : 0;
    host_block->history_capacity = history_capacity;
    return RPNET_OK;
}

namespace rpnet {

// the checks rpnet_grad_sumsq and rpnet_adam_step_guarded share; 0 or a status with the error string set
static int guard_check(const char* who, const void* table, int64_t n_chunks, const float* grad, const double* partials,
                       const rpnet_grad_guard* guard, const double* history) {
    RPNET_REQUIRE(table && grad && partials && guard, RPNET_ERR_ARG, "%s: null pointer", who);
    RPNET_REQUIRE(n_chunks >= 1 && n_chunks < kAdamMaxTotal, RPNET_ERR_SHAPE, "%s: %lld chunks", who, (long long)n_chunks);
    RPNET_REQUIRE(((uintptr_t)table % 8) == 0 && ((uintptr_t)partials % 8) == 0 && ((uintptr_t)guard % 8) == 0 &&
                      ((uintptr_t)history % 8) == 0, RPNET_ERR_ARG,
                  "%s: the table, the partial sums, the guard block and the history ring must be 8-byte aligned", who);
    RPNET_REQUIRE(((uintptr_t)grad % 4) == 0, RPNET_ERR_ARG, "%s: grad must be 4-byte aligned", who);
    const void* bufs[] = {table, grad, partials, guard, history};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            RPNET_REQUIRE(bufs[i] != bufs[j], RPNET_ERR_ARG,
                          "%s: the table, grad, the partial sums, the guard block and the history ring are five buffers", who);
    return RPNET_OK;
}

static void launch_sumsq(const rpnet_adam_chunk* table, int64_t n_chunks, const float* grad, double* partials, hipStream_t stream) {
    const int blocks = (int)(n_chunks < kAdamMaxBlocks ? n_chunks : kAdamMaxBlocks);
    if (((uintptr_t)grad % 16) == 0)
        hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(blocks), dim3(256), 0, stream, table, (long)n_chunks, grad, partials);
    else
        hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(blocks), dim3(256), 0, stream, table, (long)n_chunks, grad, partials);
}

}  // namespace rpnet

extern "C" int rpnet_grad_sumsq(const struct rpnet_adam_chunk* table, int64_t n_chunks, const float* grad, double* partials,
                                struct rpnet_grad_guard* guard, double* history, rpnet_stream_t stream) {
    using namespace rpnet;
    const int rc = guard_check("grad_sumsq", table, n_chunks, grad, partials, guard, history);
    if (rc != RPNET_OK) return rc;
    launch_sumsq(table, n_chunks, grad, partials, (hipStream_t)stream);
    rpnet_adam_hyper* no_optimizer = nullptr;
    hipLaunchKernelGGL(adam_advance_guarded_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, (long)n_chunks,
                       no_optimizer, guard, history);
    return check_launch("grad_sumsq");
}

extern "C" int rpnet_adam_step_guarded(const struct rpnet_adam_chunk* table, int64_t n_chunks, const float* grad, float* m, float* v,
                                       struct rpnet_adam_hyper* hyper, double* partials, struct rpnet_grad_guard* guard,
                                       double* history, rpnet_stream_t stream) {
    using namespace rpnet;
    RPNET_REQUIRE(m && v && hyper, RPNET_ERR_ARG, "adam_step_guarded: null pointer");
    const int rc = guard_check("adam_step_guarded", table, n_chunks, grad, partials, guard, history);
    if (rc != RPNET_OK) return rc;
    RPNET_REQUIRE(((uintptr_t)hyper % 8) == 0, RPNET_ERR_ARG, "adam_step_guarded: the hyper-parameter block must be 8-byte aligned");
    RPNET_REQUIRE(((uintptr_t)m % 4) == 0 && ((uintptr_t)v % 4) == 0, RPNET_ERR_ARG, "adam_step_guarded: m and v must be 4-byte aligned");
    RPNET_REQUIRE(grad != m && grad != v && m != v, RPNET_ERR_ARG, "adam_step_guarded: grad, m and v are three buffers");
    const void* state[] = {m, v, hyper};
    const void* work[] = {table, partials, guard, history};
    for (const void* a : state)
        for (const void* b : work)
            RPNET_REQUIRE(a != b, RPNET_ERR_ARG, "adam_step_guarded: m, v and the hyper-parameter block are buffers of their own");
    RPNET_REQUIRE((const void*)hyper != (const void*)m && (const void*)hyper != (const void*)v && (const void*)hyper != (const void*)grad,
                  RPNET_ERR_ARG, "adam_step_guarded: m, v and the hyper-parameter block are buffers of their own");
    const bool vec = ((uintptr_t)grad % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0;
    const int blocks = (int)(n_chunks < kAdamMaxBlocks ? n_chunks : kAdamMaxBlocks);
    launch_sumsq(table, n_chunks, grad, partials, (hipStream_t)stream);
    hipLaunchKernelGGL(adam_advance_guarded_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, (long)n_chunks,
                       hyper, guard, history);
    if (vec)
        hipLaunchKernelGGL((adam_update_kernel<true, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, table, (long)n_chunks,
                           grad, m, v, (const rpnet_adam_hyper*)hyper, (const rpnet_grad_guard*)guard);
    else
        hipLaunchKernelGGL((adam_update_kernel<false, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, table, (long)n_chunks,
                           grad, m, v, (const rpnet_adam_hyper*)hyper, (const rpnet_grad_guard*)guard);
    return check_launch("adam_step_guarded");
}
