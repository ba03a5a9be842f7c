/* C ABI of the optimizer entry points of librpnet_hip.so (csrc/optim.hip; rpnet_amd/optim.py).
 *
 * A header of its own beside rpnet_abi.h, after the precedent of rpnet_eval_abi.h: these entry points are additions that change nothing
 * in rpnet_abi.h (RPNET_ABI_VERSION stays 111) or in rpnet_eval_abi.h, and their ledger of tests is tests/optim_abi_ledger.py, held to
 * the rules of tests/abi_ledger.py by tests/test_host_optim_abi_ledger.py.  Status codes, rpnet_stream_t and rpnet_last_error_string()
 * are those of rpnet_abi.h.  A library that carries these symbols says so: rpnet_optim_abi_version() == RPNET_OPTIM_ABI_VERSION. */
#ifndef RPNET_OPTIM_ABI_H
#define RPNET_OPTIM_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_OPTIM_ABI_VERSION 1
int rpnet_optim_abi_version(void);

/* ------------------------------------------------- Adam over the flat gradient bucket (csrc/optim.hip; rpnet_amd/optim.py: FusedAdam)
 * The gradients of all parameters lie in ONE flat fp32 buffer (rpnet_amd/parallel.py: FlatGradBucket), the two moments m and v in two
 * more buffers of the same layout; the parameters keep their own storage.  A CHUNK TABLE, planned once on the host and uploaded once,
 * tells the update launch where each run of at most RPNET_ADAM_CHUNK elements of one parameter lies. */

/* elements per chunk: 256 lanes x 16 bytes x 4.  Part of this ABI version: every library with RPNET_OPTIM_ABI_VERSION 1 plans with
 * 4096.  (2048 and 8192 were measured once with the constant edited, profiles/optim_step.txt: no difference beyond the spread.) */
#define RPNET_ADAM_CHUNK 4096

/* one entry of the chunk table (24 bytes) */
struct rpnet_adam_chunk {
    float* param;        /* the parameter's device pointer advanced to the chunk's first element */
    int64_t flat_start;  /* index of that element in the flat gradient / m / v buffers */
    int32_t count;       /* 1 .. RPNET_ADAM_CHUNK elements, all of ONE parameter */
    int32_t vec16;       /* 1: flat_start % 4 == 0 and param is 16-byte aligned -> 16-byte loads and stores for count / 4 quads, the
                            count % 4 elements behind them one by one; 0: every element one by one */
};

/* the hyper-parameter block, 96 bytes in DEVICE memory (8-byte aligned).  The host writes the first seven fields (to change the
 * learning rate: copy 8 bytes to offset 0); the advance launch of rpnet_adam_step rewrites `step` and the fp32 fields, nothing
 * is ever read back during a step. */
struct rpnet_adam_hyper {
    double lr, beta1, beta2, eps, weight_decay, grad_scale;
    int64_t step;        /* steps taken so far; rpnet_adam_step adds one before it updates */
    /* derived by the advance launch, in fp64 as torch.optim.Adam's Python does (bc1 = 1 - beta1**step, step_size = lr / bc1,
     * bc2_sqrt = sqrt(1 - beta2**step)), then rounded to fp32 ONCE for the update.  one_minus_beta1 / one_minus_beta2 are
     * (float)(1.0 - beta): forming 1 - (float)beta in fp32 instead would be off by up to 3e-5 relative for beta2 = 0.999. */
    float step_size, bc2_sqrt, eps_f, weight_decay_f, grad_scale_f, beta1_f, beta2_f, one_minus_beta1, one_minus_beta2, reserved;
};

/* rpnet_adam_plan_bytes   bytes of the HOST buffer rpnet_adam_plan fills for n parameters of counts[i] elements (0 and an error
 *                         string when n < 1, counts is null or a count is below 1).  No GPU call.
 * rpnet_adam_plan         writes the chunk table into `table` (host memory, table_bytes >= rpnet_adam_plan_bytes) and the number of
 *                         entries into *n_chunks; the caller uploads it.  params[i]: device pointer of parameter i, counts[i] its
 *                         elements, offsets[i] its first index in the flat buffers.  No GPU call, nothing is dereferenced.  Refused
 *                         with a status and an error string: a null argument, n < 1, a null or not 4-byte aligned parameter pointer, a
 *                         count below 1, offsets[0] < 0, offsets that do not ascend or overlap (offsets[i] < offsets[i-1] +
 *                         counts[i-1]), an end offsets[n-1] + counts[n-1] of 2^40 or more, a table buffer that is too small
 *                         (RPNET_ERR_WORKSPACE).
 * rpnet_adam_step         ONE optimizer step as two launches on `stream`, no allocation, no synchronisation:
 *                         1. advance (one wave): hyper->step += 1 and the derived fp32 fields of hyper;
 *                         2. update (grid-stride over the table, at most 2048 blocks of 256), per element, all in fp32, the rounding
 *                            sequence of torch.optim.Adam(amsgrad=False, maximize=False) on the CPU (L2 weight decay):
 *                              g' = fma(weight_decay, p, grad_scale * g)
 *                              m  = fma(1 - beta1, g' - m, m)
 *                              v  = fma((1 - beta2) * g', g', beta2 * v)
 *                              p  = p + (-step_size * m) / (sqrt(v) / bc2_sqrt + eps)      (IEEE sqrt and divisions)
 *                         grad is read only; m, v: flat fp32 buffers laid out like grad; p is written through the table.  table:
 *                         DEVICE copy of the planned table, 8-byte aligned, n_chunks >= 1 entries; grad, m, v 4-byte aligned (when
 *                         one of them is not 16-byte aligned every chunk goes element by element); hyper 8-byte aligned.  The table is
 *                         trusted: every entry must lie inside the four buffers. */
size_t rpnet_adam_plan_bytes(const int64_t* counts, int n);
int rpnet_adam_plan(const void* const* params, const int64_t* counts, const int64_t* offsets, int n, void* table, size_t table_bytes,
                    int64_t* n_chunks);
int rpnet_adam_step(const struct rpnet_adam_chunk* table, int64_t n_chunks, const float* grad, float* m, float* v,
                    struct rpnet_adam_hyper* hyper, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_OPTIM_ABI_H */
