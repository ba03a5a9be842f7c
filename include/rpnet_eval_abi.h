/* C ABI of the evaluation-item entry points of librpnet_hip.so (csrc/evalitem.hip; rpnet_amd/dataset_eval.py).
 *
 * A header of its own beside rpnet_abi.h: these entry points are additions that change nothing in rpnet_abi.h (RPNET_ABI_VERSION stays
 * 111, every existing caller is served as before), and their ledger of tests is tests/eval_abi_ledger.py, held to the rules of
 * tests/abi_ledger.py by tests/test_host_eval_abi_ledger.py (header == binding == ledger; every entry names a GPU test that names
 * the symbol).  Status codes, rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h.  A library that carries these
 * symbols says so: rpnet_eval_abi_version() == RPNET_EVAL_ABI_VERSION. */
#ifndef RPNET_EVAL_ABI_H
#define RPNET_EVAL_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_EVAL_ABI_VERSION 1
int rpnet_eval_abi_version(void);

/* ------------------------------------------------- evaluation items of a data-set run (csrc/evalitem.hip; rpnet_amd/dataset_eval.py)
 * rpnet_eval_item_gather  the eval branch of the slice reader (dataset/few_shot_reader.py:523-546, one shot) in ONE launch: query
 *                         slice s of q_img / q_msk [S][H][W] is paired with slice support_slice[s] of s_img / s_msk [Ds][H][W]
 *                         (support_slice: S int32 in DEVICE memory, every entry in [0, Ds) - the caller checks the table before it
 *                         uploads it; the kernel clamps, so that a bad entry cannot read outside the volume).  Writes, each [S][H][W]:
 *                         sup_img, sup_lab, qry_img, qry_lab (copies: the tensors the model and the tallies take) and sup_reg, qry_reg
 *                         = (image + 1) / 2 as ONE fp32 add and ONE fp32 multiply by 0.5, bit-identical to the host expression (the
 *                         planes the registration takes).  16-byte accesses along W (taken on 4-byte boundaries when W % 4 != 0 or a
 *                         pointer is not 16-byte aligned), the W % 4 columns of a row one by one.  No output may alias an input or
 *                         another output.  Refused: a null pointer, Ds / S / H / W < 1, S > 65535, S*H*W or Ds*H*W >= 2^32.
 * rpnet_ncc_pairs         table[row][0] = NCC(query, warped), table[row][1] = NCC(query, affine) over n elements each, NCC(m, f) =
 *                         -sum((f - mean f)(m - mean m)) / sqrt(sum (f - mean f)^2 sum (m - mean m)^2 + 1e-10) (net/registration.py:
 *                         157-160; the two figures of test_rpnet.py:229-230).  Everything in fp64, in two passes (means, then centred
 *                         sums); per-block partial rows in `workspace`, combined in an order that depends on n alone: no atomics, two
 *                         runs give the same bits.  table: fp64 [n_rows][2] in device memory, 0 <= row < n_rows; 1 <= n < 2^29;
 *                         workspace >= rpnet_ncc_pairs_workspace_bytes(n), 8-byte aligned.  Three launches. */
int rpnet_eval_item_gather(const float* s_img, const float* s_msk, const float* q_img, const float* q_msk, const int32_t* support_slice,
                           float* sup_img, float* sup_lab, float* qry_img, float* qry_lab, float* sup_reg, float* qry_reg, int Ds, int S,
                           int H, int W, rpnet_stream_t stream);
size_t rpnet_ncc_pairs_workspace_bytes(size_t n);
int rpnet_ncc_pairs(const float* query, const float* warped, const float* affine, size_t n, double* table, int row, int n_rows,
                    void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_EVAL_ABI_H */
