/* C ABI of the component post-processing entry points of librpnet_hip.so: filling the holes of one class of a segmented volume and
 * removing its small components (csrc/cc_post.hip; rpnet_amd/postprocess.py, VolumeSegmenter(fill_holes=..., min_component=...)).
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h, rpnet_guard_abi.h, rpnet_surface_abi.h, rpnet_cc_abi.h and
 * rpnet_surface_spacing_abi.h, none of which it changes; its ledger of tests is tests/ccpost_abi_ledger.py, held to the rules of
 * tests/abi_ledger.py by tests/test_host_ccpost_abi_ledger.py.  Status codes, rpnet_stream_t and rpnet_last_error_string() are those of
 * rpnet_abi.h; element kinds, the axis limit and the component labels are those of rpnet_cc_abi.h.  A library that carries these symbols
 * says so: rpnet_ccpost_abi_version() == RPNET_CCPOST_ABI_VERSION.
 *
 * Definitions.  A volume [D][H][W], a class cls; the object is `value == cls`.
 *
 * Holes.  The complement is `value != cls`.  Two complement voxels are neighbours when they share a face (background connectivity 6)
 * or a face, an edge or a corner (26): structure = generate_binary_structure(3, 1) or (3, 3) of scipy.ndimage.binary_fill_holes, 6 being
 * scipy's default.  In per-slice mode the background connectivity is 4 or 8 (generate_binary_structure(2, 1) or (2, 2)): every z slice is
 * its own 2D image with no link across z, and the border is the slice's own four edges.  A component of the complement is a hole when
 * none of its voxels lies on the border of the volume (per slice: of its slice) and its size is <= max_hole_voxels; max_hole_voxels 0
 * means no bound.  Filling writes cls to the voxels of a hole whose value is 0; voxels of other classes inside a hole pass through
 * unchanged (and count towards the size of the hole).  With one foreground class and no bound this is binary_fill_holes.
 *
 * Small components.  The components of `value == cls` under connectivity 6 or 26, as rpnet_cc_abi.h labels them.  A component is
 * removed (its voxels set to 0) when its size is < min_voxels.  Other classes pass through unchanged.
 *
 * Everything is integer work and no result depends on the order in which blocks or atomics run: two runs give the same bits. */
#ifndef RPNET_CCPOST_ABI_H
#define RPNET_CCPOST_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_CCPOST_ABI_VERSION 1
int rpnet_ccpost_abi_version(void);

/* columns of a row of the two tables */
#define RPNET_CCPOST_STATS_ROW 4  /* int64.  rpnet_ccpost_fill_holes: n_complement_components, n_holes, voxels_filled, largest_hole
                                   * (the size of the largest hole in complement voxels, 0 without a hole).  rpnet_ccpost_remove_small:
                                   * n_components, n_removed, voxels_removed, largest_removed (0 when nothing was removed) */
#define RPNET_CCPOST_COUNTS_ROW 3 /* int64: |P and T|, |P|, |T| of the class in the result (added to what the row holds) */

/* byte offset of the `overrun` word (uint32) inside a workspace: 0 after every call unless a loop ran out of its bound; the first
 * column of the statistics row is then -1 */
#define RPNET_CCPOST_OVERRUN_OFFSET 24

/* rpnet_ccpost_workspace_bytes  bytes of device memory a call on a D x H x W volume needs (a 64-byte head, then two int32 volumes:
 *                            parent and size).  No GPU call.  0 and an error string for an extent below 1 or above RPNET_CC_MAX_DIM.
 * rpnet_ccpost_fill_holes    Launches on `stream` only; no allocation, no synchronisation, nothing read back, so a call can be captured
 *                            in a graph; the head and the size volume are cleared by the first launch:
 *                            1. to 3. local labelling, seam merge and flatten + sizes of rpnet_cc_abi.h with the complement as the
 *                               labelled set (per slice: without any link across z);
 *                            4. border: one thread per voxel of the six faces (per slice: of the four edges of every slice); a
 *                               complement voxel sets the sign bit of size[root] by an integer atomicOr of one value.  A size is at
 *                               most 2^30, so the additions of step 3 never reach that bit and the order of the two cannot matter;
 *                            5. fill and tally: a voxel whose root has a clear sign bit and a size within the bound belongs to a
 *                               hole: out[i] = in[i] == 0 ? cls : (uint8)in[i]; every other voxel passes through (as uint8).  The
 *                               roots supply the statistics; they and the three Dice counts of the result (with a truth volume)
 *                               are gathered per block before one integer atomic per block; out is written 16 bytes per lane where
 *                               it is 16-byte aligned;
 *                            6. one one-thread launch writes stats[stats_row].
 * rpnet_ccpost_remove_small  steps 1 to 3 on `value == cls` exactly as rpnet_cc_label runs them, then
 *                            4. remove and tally: out[i] = size[root] < min_voxels ? 0 : cls for the voxels of the class, every other
 *                               voxel passes through (as uint8); statistics and Dice counts as above;
 *                            5. the statistics row.
 *
 * Every loop carries its bound (the voxel count of the tile or of the volume) in its condition, as in rpnet_cc_abi.h; a loop that
 * exhausts it sets the `overrun` word and the first column of the statistics row is -1.  No spin-wait, no ticket, no cooperative launch.
 *
 * in, truth: D*H*W elements of the given kind (RPNET_CC_U8 .. RPNET_CC_F32), aligned to their element size.  out: uint8 [D][H][W]; it may
 * be `in` itself when `in` is uint8.  stats: int64 [n_rows][4], counts: int64 [n_rows][3], device memory, 8-byte aligned,
 * 0 <= stats_row, counts_row < n_rows.  truth and counts may both be null (no tally); one without the other is refused.  workspace: at
 * least rpnet_ccpost_workspace_bytes(D, H, W) bytes, 16-byte aligned, used by one call at a time.
 * Refused with a status and an error string, before anything is launched: a null pointer, an unknown kind, bg_connectivity not 6 or 26
 * (with per_slice: not 4 or 8), connectivity not 6 or 26, cls outside 1..255, max_hole_voxels < 0, min_voxels < 1, a row out of range,
 * an extent below 1 or above RPNET_CC_MAX_DIM, a workspace that is too small or misaligned, truth without counts or counts without
 * truth, `out` aliasing an `in` that is not uint8. */
size_t rpnet_ccpost_workspace_bytes(int D, int H, int W);
int rpnet_ccpost_fill_holes(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int bg_connectivity, int per_slice,
                            int64_t max_hole_voxels, const void* truth, int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats,
                            int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);
int rpnet_ccpost_remove_small(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int connectivity, int64_t min_voxels,
                              const void* truth, int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats, int64_t stats_row,
                              int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_CCPOST_ABI_H */
