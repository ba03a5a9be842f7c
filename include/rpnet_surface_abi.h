/* C ABI of the surface-distance entry points of librpnet_hip.so: the tallies behind the 95th-percentile Hausdorff distance (HD95),
 * the Hausdorff distance (HD) and the average symmetric surface distance (ASSD) of an evaluated volume (csrc/surface.hip;
 * rpnet_amd/surface.py, VolumeSegmenter(surface=True), evaluate_dataset(surface=True)).
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h and rpnet_guard_abi.h, none of which it changes; its
 * ledger of tests is tests/surface_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_surface_abi_ledger.py.
 * Status codes, rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h.  A library that carries these symbols says so:
 * rpnet_surface_abi_version() == RPNET_SURFACE_ABI_VERSION.
 *
 * Definition (the common medpy / MONAI one, in voxel units).  For a binary volume M [D][H][W], border(M) = M & ~erode(M) with the
 * 6-neighbourhood, voxels outside the volume counting as background (a foreground voxel on a volume face is a border voxel; with
 * D == 1 every foreground voxel is one).  For a prediction A and a truth B, d_AB are the Euclidean distances from every voxel of
 * border(A) to the nearest voxel of border(B), d_BA the reverse; HD = max(d_AB u d_BA), HD95 = the 95th percentile of the pooled
 * distances with linear interpolation, ASSD = (mean d_AB + mean d_BA) / 2.  With unit spacing every squared distance is an integer
 * below D^2 + H^2 + W^2, so everything below is exact integer work but the two sums of square roots. */
#ifndef RPNET_SURFACE_ABI_H
#define RPNET_SURFACE_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_SURFACE_ABI_VERSION 1
int rpnet_surface_abi_version(void);

/* largest extent per axis (a constant of this ABI version): the "no seed" value of the transform, 2^29, plus three squared extents
 * stays below 2^31 */
#define RPNET_SURFACE_MAX_DIM 1024

/* element kinds of a volume handed to rpnet_surface_tally: foreground is `value == cls` (fp32: `value == (float)cls`) */
#define RPNET_SURFACE_U8 0  /* uint8: the mask VolumeSegmenter keeps */
#define RPNET_SURFACE_I32 1 /* int32 labels */
#define RPNET_SURFACE_I64 2 /* int64 labels */
#define RPNET_SURFACE_F32 3 /* float32 0/1 planes: the affine baseline, the labels of an evaluation item */

/* columns of a row of the two tables */
#define RPNET_SURFACE_IROW 6 /* int64: n_A, n_B, d2_k, d2_k1, d2_max, k */
#define RPNET_SURFACE_FROW 2 /* fp64:  sum over border(A) of sqrt(d^2), sum over border(B) of sqrt(d^2) */

/* rpnet_surface_workspace_bytes  bytes of device memory a tally of a D x H x W volume needs.  No GPU call.  0 and an error string for
 *                        an extent below 1 or above RPNET_SURFACE_MAX_DIM.
 * rpnet_surface_tally    one prediction against one truth for one class.  Launches on `stream` only; no allocation, no
 *                        synchronisation, nothing read back; the histogram inside the workspace is cleared by a memset on `stream`:
 *                        1. x pass (both volumes, grid.y = 2): a block stages whole x lines in LDS, forms the border flags from the
 *                           two x neighbours in LDS and the four y / z neighbours in global memory, and every voxel scans outward
 *                           from its own position for the nearest border voxel of its line: squared distance, or 2^29 ("no seed");
 *                        2. y pass, 3. z pass (both volumes, grid.z = 2), in place: the exact separable min-plus transform in int32,
 *                           out[i] = min_j (in[j] + (i - j)^2).  A block stages the whole lines of a tile of neighbouring x columns
 *                           in LDS (coalesced rows; at most 32 KiB: 64 columns for lines up to 128, 32 up to 256, ... 8 up to 1024),
 *                           every voxel scans outward from its own position and stops once the squared offset alone reaches its best;
 *                           an all-background volume comes out as 2^29 everywhere;
 *                        4. histogram: border(A) voxels (transform of A == 0) add one to hist[0][d2 to border(B)], border(B) voxels
 *                           to hist[1][d2 to border(A)]; 64-bit counters, nbins = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1, the first 1024
 *                           bins gathered per block in LDS; integer atomicAdd only, so two runs give the same bits;
 *                        5. finalize (one block): n_A, n_B, n = n_A + n_B, k = floor(0.95 * (n - 1)) in fp64 as numpy's percentile
 *                           forms it, d2_k and d2_k1 the k-th and min(k + 1, n - 1)-th smallest squared distance of the pooled
 *                           histogram, d2_max the largest, into itable[irow]; sum_bins count * sqrt((double)bin) of either
 *                           histogram, in a fixed order without floating-point atomics, into ftable[frow].  When n_A == 0 or
 *                           n_B == 0 every column of both rows is 0 and k = -1.
 *                        Every loop has a bound known at entry; no spin-wait; blocks share nothing but the integer atomicAdd of 4.
 * pred, truth: D*H*W elements of the given kind, aligned to their element size.  itable: int64 [n_rows][RPNET_SURFACE_IROW], ftable:
 * fp64 [n_rows][RPNET_SURFACE_FROW], both in device memory and 8-byte aligned, 0 <= irow, frow < n_rows.  workspace: at least
 * rpnet_surface_workspace_bytes(D, H, W) bytes, 16-byte aligned, used by one tally at a time.  Refused with a status and an error string,
 * before anything is launched: a null pointer, an unknown kind, a row out of range, an extent below 1 or above RPNET_SURFACE_MAX_DIM, a
 * workspace that is too small or misaligned. */
size_t rpnet_surface_workspace_bytes(int D, int H, int W);
int rpnet_surface_tally(const void* pred, int pred_kind, const void* truth, int truth_kind, int cls, int D, int H, int W, int64_t* itable,
                        int64_t irow, double* ftable, int64_t frow, int64_t n_rows, void* workspace, size_t workspace_bytes,
                        rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_SURFACE_ABI_H */
