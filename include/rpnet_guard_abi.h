/* C ABI of the gradient guard of librpnet_hip.so: the gradient norm, norm clipping and the non-finite skip inside the Adam step
 * (csrc/optim.hip; rpnet_amd/optim.py: FusedAdam(max_grad_norm=, skip_nonfinite=, history=)).
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h and rpnet_optim_abi.h, none of which it changes; its ledger of tests is
 * tests/guard_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_guard_abi_ledger.py.  Status codes,
 * rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h, the chunk table and the hyper-parameter block those of
 * rpnet_optim_abi.h.  A library that carries these symbols says so: rpnet_guard_abi_version() == RPNET_GUARD_ABI_VERSION. */
#ifndef RPNET_GUARD_ABI_H
#define RPNET_GUARD_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_optim_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_GUARD_ABI_VERSION 1
int rpnet_guard_abi_version(void);

/* the guard block, 80 bytes in DEVICE memory (8-byte aligned).  The host writes the first three fields (rpnet_grad_guard_init fills
 * a host copy with everything else zero; to change the threshold later: copy 8 bytes to offset 0); the launches below write the rest,
 * nothing is ever read back during a step. */
struct rpnet_grad_guard {
    double max_norm;           /* clip threshold of the gradient's 2-norm, > 0; +inf: no clipping */
    int64_t skip_nonfinite;    /* != 0: a step whose sum of squares is inf or NaN is not taken */
    int64_t history_capacity;  /* rows of the history ring handed to the calls below, 0: none */
    double sumsq;              /* sum of g^2 over every element of the chunk table, BEFORE grad_scale */
    double norm;               /* |grad_scale| * sqrt(sumsq): the norm of the gradient the update sees */
    double coef;               /* c = max_norm / (norm + 1e-6), c when c <= 1 or c is NaN, else 1: torch.nn.utils.clip_grad_norm_'s */
    float coef_f;              /* (float)coef of the last step that was taken: what the update multiplies by */
    int32_t skip;              /* 1: the last attempt was skipped */
    int64_t attempt;           /* calls so far, skipped ones included */
    int64_t skipped;           /* steps not taken */
    int64_t clipped;           /* steps taken with coef < 1 */
};
#ifdef __cplusplus
static_assert(sizeof(struct rpnet_grad_guard) == 80, "rpnet_grad_guard is 80 bytes");
#else
_Static_assert(sizeof(struct rpnet_grad_guard) == 80, "rpnet_grad_guard is 80 bytes");
#endif

/* one row of the history ring: RPNET_GUARD_HISTORY_ROW doubles (norm, coef, skip as 0.0 / 1.0).  Attempt number a (counted from 0)
 * goes to row a % history_capacity, so the ring holds the last history_capacity attempts. */
#define RPNET_GUARD_HISTORY_ROW 3

/* rpnet_grad_guard_init   fills a HOST copy of the block: the three host-written fields from the arguments, every other field zero;
 *                         the caller uploads it.  No GPU call.  Refused with a status and an error string: a null block, a max_norm
 *                         that is <= 0 or NaN, a negative history_capacity.  (These two live in device memory during a step, and a
 *                         step reads nothing back: they are checked here, where the host writes them.)
 * rpnet_grad_sumsq        the norm alone, two launches on `stream`, no allocation, no synchronisation, no atomics:
 *                         1. sum of squares (grid-stride over the table, at most 2048 blocks of 256, a chunk per block iteration):
 *                            every lane squares and adds in fp64 (the square of an fp32 value is exact in fp64), lanes, the wave
 *                            and the four waves are added in a fixed order, one double per chunk into partials[n_chunks]: the
 *                            result depends on neither the grid size nor timing, and covers exactly the elements the update touches;
 *                         2. record (one block): adds the partials in a fixed order, writes sumsq, norm = sqrt(sumsq) (no
 *                            grad_scale: there is no optimizer here), coef, coef_f and skip = (skip_nonfinite and sumsq not finite)
 *                            into the guard, norm / coef / skip into row attempt % history_capacity of `history` when history is not
 *                            null and history_capacity > 0, and adds one to attempt.  skipped and clipped are left alone.
 * rpnet_adam_step_guarded ONE guarded optimizer step as three launches on `stream`, no allocation, no synchronisation, no atomics:
 *                         1. sum of squares, as above;
 *                         2. advance (one block): sumsq, norm = |hyper->grad_scale| * sqrt(sumsq), coef, the history row and attempt
 *                            as above; when skip_nonfinite and sumsq is not finite: skip = 1, skipped += 1, hyper is left as it is;
 *                            otherwise skip = 0, coef_f = (float)coef, clipped += 1 when coef < 1, and the advance of
 *                            rpnet_adam_step (hyper->step += 1, the derived fp32 fields).  With skip_nonfinite == 0 a non-finite
 *                            sum does what clip_grad_norm_(error_if_nonfinite=False) does: a NaN sum gives a NaN coefficient and
 *                            NaN parameters;
 *                         3. update: nothing at all when skip is set (not one byte of p, m, v is written); otherwise the update of
 *                            rpnet_adam_step with g' = fma(weight_decay, p, coef_f * (grad_scale * g)), the two products rounded in
 *                            that order (flat.mul_(scale), then clip_grad_norm_'s g.mul_(coef)).  coef_f == 1 multiplies exactly:
 *                            a guarded step that neither clips nor skips is bit-identical to rpnet_adam_step.
 *                         grad is read only: unlike clip_grad_norm_, the bucket is NOT rewritten with the clipped gradient.
 * table, n_chunks, grad, m, v, hyper: as for rpnet_adam_step.  partials: n_chunks doubles of device memory, 8-byte aligned, overwritten
 * by every call.  guard: device copy of the block, 8-byte aligned.  history: null, or RPNET_GUARD_HISTORY_ROW * history_capacity
 * doubles of device memory, 8-byte aligned.  Refused with a status and an error string: a null pointer (history excepted), n_chunks
 * < 1, a misaligned pointer, two of the buffers at the same address. */
int rpnet_grad_guard_init(struct rpnet_grad_guard* host_block, double max_norm, int skip_nonfinite, int64_t history_capacity);
int rpnet_grad_sumsq(const struct rpnet_adam_chunk* table, int64_t n_chunks, const float* grad, double* partials,
                     struct rpnet_grad_guard* guard, double* history, rpnet_stream_t stream);
int rpnet_adam_step_guarded(const struct rpnet_adam_chunk* table, int64_t n_chunks, const float* grad, float* m, float* v,
                            struct rpnet_adam_hyper* hyper, double* partials, struct rpnet_grad_guard* guard, double* history,
                            rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_GUARD_ABI_H */
