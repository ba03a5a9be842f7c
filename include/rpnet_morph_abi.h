/* C ABI of the ball-morphology entry points of librpnet_hip.so: erosion, dilation, opening and closing of one class of a segmented
 * volume by a Euclidean ball in voxels or by the ellipsoid of voxels within r under a per-axis spacing (csrc/morph.hip;
 * rpnet_amd/morphology.py, VolumeSegmenter(opening=..., closing=...)).
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h, rpnet_guard_abi.h, rpnet_surface_abi.h, rpnet_cc_abi.h,
 * rpnet_surface_spacing_abi.h and rpnet_ccpost_abi.h, none of which it changes; its ledger of tests is tests/morph_abi_ledger.py, held to
 * the rules of tests/abi_ledger.py by tests/test_host_morph_abi_ledger.py.  Status codes, rpnet_stream_t and rpnet_last_error_string()
 * are those of rpnet_abi.h; element kinds and the axis limit are those of rpnet_cc_abi.h.  A library that carries these symbols says so:
 * rpnet_morph_abi_version() == RPNET_MORPH_ABI_VERSION.
 *
 * Definitions.  A volume [D][H][W] (the set of its voxels is Omega), a class cls; the object is X = (value == cls).
 *
 * Voxel ball.  A squared radius rho, an integer >= 1: B = {(dz,dy,dx) : dz^2 + dy^2 + dx^2 <= rho}.  rho = 1, 2, 3 are
 * scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3), the 6-, 18- and 26-neighbourhoods; a radius r in voxels means rho = floor(r^2).
 * Per-slice mode takes dz = 0 only: every z slice is its own 2D image, as in rpnet_ccpost_fill_holes.
 *
 * Millimetre ball.  Weights w = {wz, wy, wx} (the squares s * s of a spacing, rounded once) and a squared radius r2 = fl(r * r), all
 * doubles: B = {o : fl(fl(fl(wx * dx^2) + fl(wy * dy^2)) + fl(wz * dz^2)) <= r2}: the operations of rpnet_surface_spacing_tally in
 * the order its x, y and z passes apply them, every product and every sum one rounding, so a numpy restatement gets the same set.
 *
 * Operations on Omega.
 *   dilate(X) = {v in Omega : there is s in X with v - s in B}; outside Omega is background.
 *   erode(X)  = {v in Omega : for every o in B, v + o in X or v + o not in Omega}; outside Omega counts as object
 *               (border_value=1 of scipy.ndimage.binary_erosion).  With this adjoint pair close = erode . dilate is extensive and
 *               idempotent and open = dilate . erode anti-extensive and idempotent on a bounded volume.
 *   erode_border = 0: outside Omega counts as background in every erosion of the call (scipy's default border_value=0; its
 *               binary_closing then eats objects that touch the border, and so does this).  In closed form: a voxel is also eroded
 *               when an outside voxel along one of the axes lies within the ball (per slice: along y or x only).
 * The route: dilate(X) = {v : d2(v, X) <= rho} and erode(X) = {v : d2(v, Omega \ X) > rho}, d2 the separable distance transform of
 * csrc/surface_edt.h under the same metric, capped at the first value above rho.
 *
 * Writing back into a label volume (the rule of rpnet_ccpost_fill_holes).  Voxels the operation gains take cls only where the value is
 * 0; voxels it loses become 0; every other value passes through as uint8.
 *
 * Everything is integer or separately rounded fp64 work with integer atomics only: two runs give the same bits.
 * Not claimed: parity with SimpleITK's BinaryBall structuring element, which ITK rasterises as an ellipsoid by its own rule. */
#ifndef RPNET_MORPH_ABI_H
#define RPNET_MORPH_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_MORPH_ABI_VERSION 1
int rpnet_morph_abi_version(void);

/* op */
#define RPNET_MORPH_ERODE 0
#define RPNET_MORPH_DILATE 1
#define RPNET_MORPH_OPEN 2  /* dilate(erode(X)) */
#define RPNET_MORPH_CLOSE 3 /* erode(dilate(X)) */

#define RPNET_MORPH_MAX_RHO 3145728 /* 3 * RPNET_CC_MAX_DIM^2: the squared diagonal of the largest volume */

/* columns of a row of the two tables */
#define RPNET_MORPH_STATS_ROW 4  /* int64: voxels_before, voxels_after, voxels_added, voxels_removed of the class (written).  On a label
                                  * volume `added` can be smaller than the binary operation's gain */
#define RPNET_MORPH_COUNTS_ROW 3 /* int64: |P and T|, |P|, |T| of the class in the result (added to what the row holds) */

/* rpnet_morph_workspace_bytes  bytes of device memory a call on a D x H x W volume needs (a 64-byte head, one volume of 8-byte
 *                            transform values and two uint8 volumes, each rounded up to 16 bytes), for either ball.  No GPU call.
 *                            0 and an error string for an extent below 1 or above RPNET_CC_MAX_DIM.
 * rpnet_morph_apply          the voxel ball.  Launches on `stream` only; no allocation, no synchronisation, nothing read back, so a
 *                            call can be captured in a graph.  One transform per erosion or dilation (two for open and close):
 *                            1. seeded x pass: per voxel the cost of the nearest seed of its line (the seeds are X for a dilation,
 *                               Omega \ X for an erosion), scanned only while cost(o) <= rho; rho + 1 (the cap) without one.  Its
 *                               first launch also clears the head;
 *                            2. y pass, 3. z pass: out[i] = min(in[i], cap, min_j (in[j] + cost(i - j))) over lines staged in LDS,
 *                               each scan ending at cost(o) >= best; an axis of length 1 has no pass, per-slice mode no z pass;
 *                               the last pass of a transform writes the uint8 result instead of distances (<= rho for a dilation,
 *                               > rho and the erode_border rule for an erosion).  The second transform of open / close reads the
 *                               uint8 result of the first;
 *                            4. write back and tally: the label-volume rule, the statistics and the three Dice counts of the result
 *                               (with a truth volume) gathered per block before one integer atomic per block; out is written 16
 *                               bytes per lane where it is 16-byte aligned;
 *                            5. one one-thread launch writes stats[stats_row].
 *                            Every loop has a bound that is fixed when it is entered.
 * rpnet_morph_apply_spacing  the millimetre ball, in fp64: w = {wz, wy, wx} (host memory, read before the call returns) and r2.
 *
 * in, truth: D*H*W elements of the given kind (RPNET_CC_U8 .. RPNET_CC_F32), aligned to their element size.  out: uint8 [D][H][W]; it may
 * be `in` itself when `in` is uint8.  stats: int64 [n_rows][4], counts: int64 [n_rows][3], device memory, 8-byte aligned,
 * 0 <= stats_row, counts_row < n_rows.  truth and counts may both be null (no tally); one without the other is refused.  workspace: at
 * least rpnet_morph_workspace_bytes(D, H, W) bytes, 16-byte aligned, used by one call at a time.
 * Refused with a status and an error string, before anything is launched: a null pointer, an unknown kind or op, rho < 1 or above
 * RPNET_MORPH_MAX_RHO, a weight or r2 that is not finite or not positive, cls outside 1..255, a row out of range, an extent below 1 or
 * above RPNET_CC_MAX_DIM, a workspace that is too small or misaligned, truth without counts or counts without truth, `out` aliasing an
 * `in` that is not uint8. */
size_t rpnet_morph_workspace_bytes(int D, int H, int W);
int rpnet_morph_apply(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int op, int64_t rho, int per_slice,
                      int erode_border, const void* truth, int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats,
                      int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);
int rpnet_morph_apply_spacing(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int op, const double* w, double r2,
                              int per_slice, int erode_border, const void* truth, int truth_kind, int64_t* counts, int64_t counts_row,
                              int64_t* stats, int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes,
                              rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_MORPH_ABI_H */
