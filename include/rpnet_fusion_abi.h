/* C ABI of the label-fusion entry points of librpnet_hip.so: one mask from the masks R raters gave one volume, by majority vote, weighted
 * vote or binary STAPLE (Warfield, Zou, Wells 2004), class by class (csrc/fusion.hip; rpnet_amd/fusion.py).
 *
 * A header of its own beside rpnet_abi.h and the thirteen side headers before it, none of which it changes; its ledger of tests is
 * tests/fusion_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_fusion_abi_ledger.py.  Status codes,
 * rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h; element kinds and the largest extent are those of
 * rpnet_cc_abi.h.  A library that carries these symbols says so: rpnet_fusion_abi_version() == RPNET_FUSION_ABI_VERSION.
 *
 * Definitions.  Every float64 operation named below is rounded once (no contraction), so a numpy restatement gives the same bits
 * (tests/fusion_cases.py).
 *   raters      R volumes [D][H][W] of one element kind, 1 <= R <= RPNET_FUSION_MAX_RATERS
 *   d_r(i)      = (rater_r[i] == cls)                      (fp32: == (float)cls)
 *   pat(i)      = sum_r d_r(i) << r                         uint16: rater 0 is bit 0
 *   hist[p]     = the number of voxels with pat == p        int64 [2^R], integer atomics only
 *   d_r(p)      = bit r of p;  pc(p) = popcount(p);  full = 2^R - 1
 *   a decision table: label[p] in {0, 1} (uint8) and w[p] (float64), 0 <= p < 2^R
 *
 * VOTE      label[p] = pc(p) >= min_votes, 1 <= min_votes <= R;  w[p] = (double)pc(p) / (double)R.
 * WEIGHTED  weights: R float64, finite, >= 0, total > 0.  s[p] = the sum of the weights of the set bits of p in ascending r, from 0.0;
 *           total = s[full];  label[p] = (2 * s[p] > total)  (the doubling is exact);  w[p] = s[p] / total.
 * STAPLE    A bin participates unless consensus != 0 and p is 0 or full; those two then get label 0 / 1 and w 0.0 / 1.0 directly.
 *           n = sum of hist over the participating bins, num = sum hist[p] * pc(p) over them, both in integers;
 *           g = (double)num / (double)(R * n).  Start p_r = q_r = 0.99999.  An iteration:
 *             E   for every participating bin:  a = g, then for r ascending a = a * (d_r(p) ? p_r : 1 - p_r);
 *                 b = 1 - g, then for r ascending b = b * (d_r(p) ? 1 - q_r : q_r);  w[p] = a / (a + b)
 *             M   with h = (double)hist[p], hw = h * w[p], hv = h * (1 - w[p]):
 *                 S1 = SUM hw, S0 = SUM hv, P_r = SUM over bins with d_r(p) of hw, Q_r = SUM over bins without d_r(p) of hv;
 *                 p_r' = clamp(P_r / S1), q_r' = clamp(Q_r / S0), clamp to [2^-20, 1 - 2^-20]; a parameter whose denominator is 0
 *                 keeps its value.  delta = max_r max(|p_r' - p_r|, |q_r' - q_r|).
 *           The EM stops after max_iter iterations or after the first with delta < tol (`converged`).  label[p] = (w[p] >= 0.5) with
 *           the w of the last E step; p_r, q_r are those of the last M step.
 *           SUM is the order of the one block of 256 threads that runs the EM: thread t adds, from 0.0, the terms of the participating
 *           bins t, t + 256, t + 512, ... in ascending order; then the 256 partials are folded by a stride-halving tree,
 *           part[t] = part[t] + part[t + s] for t < s, s = 128, 64, ..., 1.  A bin that does not take part in a sum adds nothing.
 *           If n == 0 or R == 1 the table is that of VOTE with min_votes = R, iterations = 0 and the rows are those of VOTE.
 *
 * Rows.  stats[row], int64 [RPNET_FUSION_STATS_ROW]: n_participating (n above; every voxel under VOTE and WEIGHTED), n_fused
 *   = sum hist[p] * label[p], n_all_agree_fg = hist[full], n_disagree = voxels - hist[0] - hist[full], iterations, converged (1 where
 *   no EM ran).  rater_i[row], int64 [R][3]: |rater_r and fused|, |rater_r|, |fused|, with fused = label[pat], all from hist and label.
 *   rater_f[row], float64 [R][2]: p_r, q_r of the EM; where no EM ran the sensitivity |rater_r and fused| / |fused| and the specificity
 *   |not rater_r and not fused| / |not fused| against the table's mask, one division of two integers each, 1.0 where the denominator
 *   is 0.  The rows describe the table: under merge != 0 the mask written can hold fewer voxels of the class than n_fused.
 *
 * Workspace (bytes, B = 2^R, n = D*H*W):   head 64 | hist int64 [B] | w float64 [B] | label uint8 [B up to 16] | patterns uint16 [n]
 *   rpnet_fusion_workspace_bytes = 64 + 16 * B + up16(B) + up16(2 * n),  up16(x) = (x + 15) / 16 * 16
 * so a caller can read the histogram, the table and the patterns of the last call at those offsets. */
#ifndef RPNET_FUSION_ABI_H
#define RPNET_FUSION_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_FUSION_ABI_VERSION 1
int rpnet_fusion_abi_version(void);

#define RPNET_FUSION_MAX_RATERS 12  /* a pattern fits uint16 and a block's uint32 histogram 16 KiB of LDS */
#define RPNET_FUSION_MAX_ITER 100000 /* 1 <= max_iter <= 100000 */

#define RPNET_FUSION_VOTE 0
#define RPNET_FUSION_WEIGHTED 1
#define RPNET_FUSION_STAPLE 2

#define RPNET_FUSION_STATS_ROW 6  /* int64: n_participating, n_fused, n_all_agree_fg, n_disagree, iterations, converged */
#define RPNET_FUSION_COUNTS_ROW 3 /* int64: |P and T|, |P|, |T| of the class in the result (added to what the row holds) */
#define RPNET_FUSION_HEAD_BYTES 64

/* The entry points launch on `stream` only: no allocation, no synchronisation, nothing read back, so every call can be captured in a
 * graph.  Integer atomics only, no floating-point atomic anywhere; no block waits for another, no cooperative launch; the launch
 * boundaries are the only synchronisation between the passes; every loop runs to a count fixed when it is entered.  Two runs give
 * the same bits.
 *
 * rpnet_fusion_workspace_bytes  the formula above; no GPU call; 0 and an error string for an extent outside 1..RPNET_CC_MAX_DIM or R
 *                         outside 1..RPNET_FUSION_MAX_RATERS.
 * rpnet_fusion_patterns   pass 1.  `raters` is a HOST array of R device pointers; they reach the kernel by value.  A memset clears hist,
 *                         then one launch writes patterns[i] = pat(i) and fills hist: a lane owns 16 consecutive voxels (16-byte
 *                         accesses where aligned), a block of 256 lanes counts in a uint32 histogram in LDS (pattern 0 and pattern
 *                         `full` once per wave from the wave's ballot) and adds its non-zero bins to hist by 64-bit integer atomicAdd.
 *                         At most 1024 blocks; beyond that a block makes further trips, a count fixed at the launch.
 * rpnet_fusion_fuse       pass 1 into the workspace; the decision kernel, one launch of one block, which fills the table and
 *                         stats[row], rater_f[row], rater_i[row]; pass 2, which writes
 *                           merge == 0:  out[i] = label[pat(i)] ? cls : 0
 *                           merge != 0:  out[i] = (out[i] == 0 && label[pat(i)]) ? cls : out[i]
 *                           prob[i] = (float)w[pat(i)]                                       where prob is not null
 *                         and, with truth, ADDS |P and T|, |P|, |T| (P: out == cls after the write, T: truth == cls) to
 *                         counts[counts_row] by integer atomics, gathered per block first.
 *
 * raters[r], truth: D*H*W elements of their kind, aligned to the element.  patterns: uint16 [D][H][W], 2-byte aligned.  hist: int64
 * [2^R], 8-byte aligned.  out: uint8 [D][H][W].  prob: float32 [D][H][W] or null.  weights: a HOST array of R float64, read only
 * under WEIGHTED (null otherwise is fine).  stats int64 [n_rows][6], rater_f float64 [n_rows][R][2], rater_i int64 [n_rows][R][3],
 * counts int64 [n_rows][3]: device memory, 8-byte aligned, 0 <= row, counts_row < n_rows.  truth and counts may both be null; one
 * without the other is refused.  workspace: at least rpnet_fusion_workspace_bytes(D, H, W, R) bytes, 16-byte aligned, used by one call
 * at a time.  min_votes is read under VOTE, consensus, max_iter and tol under STAPLE; all are checked in every call.
 * Refused with a status and an error string, before anything is launched: a null pointer where one is required, R outside 1..12, an
 * unknown kind or method, cls outside 1..255, min_votes outside 1..R, weights missing, negative, not finite or all zero under
 * WEIGHTED, max_iter outside 1..RPNET_FUSION_MAX_ITER, tol negative or NaN, a row out of range, truth without counts or the reverse,
 * an extent out of range, a workspace that is too small or misaligned, a misaligned pointer, `out` overlapping a rater. */
size_t rpnet_fusion_workspace_bytes(int D, int H, int W, int R);
int rpnet_fusion_patterns(const void* const* raters, int R, int kind, int cls, int D, int H, int W, uint16_t* patterns, int64_t* hist,
                          rpnet_stream_t stream);
int rpnet_fusion_fuse(const void* const* raters, int R, int kind, int cls, int D, int H, int W, int method, int min_votes,
                      const double* weights, int consensus, int max_iter, double tol, uint8_t* out, int merge, float* prob, const void* truth,
                      int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats, double* rater_f, int64_t* rater_i, int64_t row,
                      int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_FUSION_ABI_H */
