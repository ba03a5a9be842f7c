/* C ABI of the surface-distance entry points of librpnet_hip.so for a grid with a per-axis voxel spacing: the tallies behind HD95, HD,
 * ASSD and the normalised surface Dice (NSD) of an evaluated volume in millimetres (csrc/surface_spacing.hip;
 * rpnet_amd/surface_spacing.py, VolumeSegmenter(surface=True, spacing=...), evaluate_dataset(surface=True, spacing=...)).
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h, rpnet_guard_abi.h, rpnet_surface_abi.h and
 * rpnet_cc_abi.h, none of which it changes; its ledger of tests is tests/surface_spacing_abi_ledger.py, held to the rules of
 * tests/abi_ledger.py by tests/test_host_surface_spacing.py.  Status codes, rpnet_stream_t and rpnet_last_error_string() are those of
 * rpnet_abi.h.  A library that carries these symbols says so: rpnet_surface_spacing_abi_version() == RPNET_SURFACE_SPACING_ABI_VERSION.
 *
 * Definition: the one at the top of rpnet_surface_abi.h (6-neighbourhood border, voxels outside the volume are background, distances
 * pooled over border(A) -> border(B) and back), with the distance between two voxels sqrt(w[0]*dz^2 + w[1]*dy^2 + w[2]*dx^2) for
 * weights w = {sz*sz, sy*sy, sx*sx} formed once by the caller from the spacing of the axes [D][H][W].
 *
 * Arithmetic.  The squared distance of a voxel is ((w[2]*dx^2 + w[1]*dy^2) + w[0]*dz^2) minimised over the border voxels, every
 * product and every sum one separately rounded fp64 operation (no fused multiply-add) and every dx^2, dy^2, dz^2 an exact integer, so a
 * restatement that performs the same operations in any order of candidates gets the same bits. */
#ifndef RPNET_SURFACE_SPACING_ABI_H
#define RPNET_SURFACE_SPACING_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_SURFACE_SPACING_ABI_VERSION 1
int rpnet_surface_spacing_abi_version(void);

/* largest extent per axis and the element kinds of a volume: those of rpnet_surface_abi.h (RPNET_SURFACE_MAX_DIM, RPNET_SURFACE_U8 /
 * I32 / I64 / F32: 0 uint8, 1 int32, 2 int64, 3 float32; foreground is `value == cls`) */
#define RPNET_SURFACE_SPACING_MAX_DIM 1024

/* columns of a row of the two tables */
#define RPNET_SURFACE_SPACING_IROW 5 /* int64: n_A, n_B, k, within_A, within_B */
#define RPNET_SURFACE_SPACING_FROW 5 /* fp64:  d2_k, d2_k1, d2_max, sum over border(A) of sqrt(d2), sum over border(B) of sqrt(d2) */

/* rpnet_surface_spacing_workspace_bytes  bytes of device memory a tally of a D x H x W volume needs: a head of counters, radix
 *                        histograms and per-block partial sums (66048 bytes), then two fp64 volumes.  No GPU call.  0 and an error
 *                        string for an extent below 1 or above RPNET_SURFACE_SPACING_MAX_DIM.
 * rpnet_surface_spacing_tally  one prediction against one truth for one class.  Launches on `stream` only; no allocation, no
 *                        synchronisation, nothing read back; the counters and histograms of the head are cleared on `stream` by the
 *                        first launch (a fill kernel rather than a memset node, so that a captured tally replays with the same bits);
 *                        the number and the shape of the launches depend on (D, H, W) alone:
 *                        1. x pass (both volumes, grid.y = 2): the border flags exactly as rpnet_surface_tally forms them; every voxel
 *                           gets w[2] * (o*o) for the nearest border voxel of its line at offset o, or the "no seed" value DBL_MAX;
 *                        2. y pass (w[1]), 3. z pass (w[0]), both volumes (grid.z = 2), in place: out[i] = min_j (in[j] + w*(i-j)^2)
 *                           in fp64, product and sum rounded separately.  A block stages the whole lines of a tile of neighbouring x
 *                           columns in LDS: 32 columns for lines up to 128, 16 up to 256, 8 up to 1024 (at most 32 KiB up to 512,
 *                           64 KiB beyond; never more than a launch gets without asking); every voxel scans outward from its own
 *                           position and stops once w*o^2 alone reaches its best.  An all-background volume keeps DBL_MAX everywhere;
 *                        4. statistics: n_A, n_B, the counts of border voxels with d2 <= tau2, the largest d2 (integer atomics on
 *                           counters and on the bit pattern); per-block partial sums of sqrt(d2) written by block index;
 *                        5. eight radix passes of 8 bits, most significant first, over the bit patterns of the pooled squared
 *                           distances (non-negative doubles order like their bit patterns read as uint64): each pass reads the
 *                           histogram of the one before, narrows the prefixes of rank k and of rank min(k + 1, n - 1), which may lie
 *                           in different buckets and are followed separately, and counts the next digit of the matching values
 *                           (integer atomicAdd, gathered per block in LDS);
 *                        6. finalize (one block): the last digit of either rank; k = floor(0.95 * (n - 1)) in fp64 as numpy's
 *                           percentile forms it; the partial sums combined in index order; {n_A, n_B, k, within_A, within_B} into
 *                           itable[irow], {d2_k, d2_k1, d2_max, sum_A, sum_B} into ftable[frow].  When n_A == 0 or n_B == 0 every
 *                           column of both rows is 0 and k = -1.
 *                        Every loop has a bound known at entry; no spin-wait; blocks share nothing but integer atomics; no
 *                        floating-point atomics, so two runs give the same bits in both rows.
 * w: three weights in host memory, in the order of the axes [D][H][W], each finite and > 0 (and small enough that 3 * w * 1023^2
 * stays finite, or the figures mean nothing).  tau2: the squared NSD tolerance, compared as d2 <= tau2; a negative tau2 means "not asked" and leaves both
 * `within` columns 0.  pred, truth, itable, ftable, the rows and the workspace: as for rpnet_surface_tally, with the widths above.
 * Refused with a status and an error string, before anything is launched: everything rpnet_surface_tally refuses (a null pointer, `w`
 * included, an unknown kind, a row out of range, an extent below 1 or above the limit, a workspace that is too small or misaligned), a
 * weight that is not finite or not > 0, a tau2 that is NaN. */
size_t rpnet_surface_spacing_workspace_bytes(int D, int H, int W);
int rpnet_surface_spacing_tally(const void* pred, int pred_kind, const void* truth, int truth_kind, int cls, int D, int H, int W,
                                const double* w, double tau2, int64_t* itable, int64_t irow, double* ftable, int64_t frow, int64_t n_rows,
                                void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_SURFACE_SPACING_ABI_H */
