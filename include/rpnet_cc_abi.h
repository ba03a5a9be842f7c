/* C ABI of the connected-component entry points of librpnet_hip.so: labelling of one class of a segmented volume and the filter that
 * keeps only the largest component of that class (csrc/components.hip; rpnet_amd/components.py, VolumeSegmenter(keep_largest=...),
 * evaluate_dataset(keep_largest=...)).
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h, rpnet_guard_abi.h and rpnet_surface_abi.h, none of
 * which it changes; its ledger of tests is tests/cc_abi_ledger.py, held to the rules of tests/abi_ledger.py by
 * tests/test_host_cc_abi_ledger.py.  Status codes, rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h.  A library
 * that carries these symbols says so: rpnet_cc_abi_version() == RPNET_CC_ABI_VERSION.
 *
 * Definition.  A volume [D][H][W]; foreground is `value == cls`; two foreground voxels are neighbours when they share a face
 * (connectivity 6) or a face, an edge or a corner (connectivity 26); voxels outside the volume are background.  A component is a class
 * of the transitive closure.  labels (int32 [D][H][W]): background 0, a foreground voxel 1 + the smallest linear index
 * z*H*W + y*W + x of its component.  That does not depend on the order in which blocks or atomics run: two runs give the same bits.
 * The largest component is the one with the most voxels; among equals the one whose first voxel comes first in z-major order, which
 * is np.argmax(np.bincount(lab.ravel())[1:]) on a scipy.ndimage.label result.  Everything is integer work. */
#ifndef RPNET_CC_ABI_H
#define RPNET_CC_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_CC_ABI_VERSION 1
int rpnet_cc_abi_version(void);

/* largest extent per axis (a constant of this ABI version; the limit of the surface ABI): a volume has at most 2^30 voxels, so a
 * linear index and a component size fit int32 */
#define RPNET_CC_MAX_DIM 1024

/* element kinds of a volume (the values of rpnet_surface_abi.h): foreground is `value == cls` (fp32: `value == (float)cls`) */
#define RPNET_CC_U8 0  /* uint8: the mask VolumeSegmenter keeps */
#define RPNET_CC_I32 1 /* int32 labels */
#define RPNET_CC_I64 2 /* int64 labels */
#define RPNET_CC_F32 3 /* float32 0/1 planes */

/* columns of a row of the two tables */
#define RPNET_CC_STATS_ROW 4  /* int64: n_foreground, n_components, size_largest, first_index_largest (0, 0, 0, -1: empty class) */
#define RPNET_CC_COUNTS_ROW 3 /* int64: |P and T|, |P|, |T| of the filtered class (added to what the row holds) */

/* byte offset of the `overrun` word (uint32) inside a workspace: 0 after every call unless a loop ran out of its bound (below) */
#define RPNET_CC_OVERRUN_OFFSET 24

/* rpnet_cc_workspace_bytes  bytes of device memory a call on a D x H x W volume needs (a 64-byte head, then two int32 volumes: parent
 *                        and size).  No GPU call.  0 and an error string for an extent below 1 or above RPNET_CC_MAX_DIM.
 * rpnet_cc_label         phases 1 to 5 below for one class.  Launches on `stream` only; no allocation, no synchronisation, nothing
 *                        read back; the head and the size volume inside the workspace are cleared by memsets on `stream`:
 *                        1. local labelling: a block of 256 threads owns a tile of 4 x 32 x 64 voxels (z, y, x: a wave reads one
 *                           whole x run of 64 voxels, 32 KiB of int32 labels in LDS).  The x runs are labelled from the wave's
 *                           foreground ballot (a voxel starts at the first voxel of its run), the runs are joined across y and z
 *                           inside the tile by union-find in LDS with the smaller index as the root (atomicMin), and every voxel
 *                           writes parent[i]: the global linear index of its root in the tile, -1 for background;
 *                        2. seam merge: every foreground voxel whose neighbour (of the lower half of the neighbourhood: 3 of 6,
 *                           13 of 26) lies in another tile unites the two roots: find by device-scope atomic loads, link by
 *                           atomicMin on parent[larger root];
 *                        3. flatten and 4. sizes, one launch: parent[i] = find(i) in place (and labels[i] = 1 + find(i), 0 for
 *                           background, where labels are asked for), size[root] += 1 by integer atomicAdd, gathered per block in a
 *                           small LDS table first; n_foreground likewise;
 *                        5. choose: every root forms the key (size << 32) | (0xFFFFFFFF - root); integer atomicMax per block in
 *                           LDS, then one per block on the head; n_components likewise by atomicAdd; one more one-thread launch
 *                           writes the statistics row stats[stats_row].
 * rpnet_cc_keep_largest  phases 1 to 5 (no labels are written), then
 *                        6. filter and tally: out[i] = parent[i] == chosen root ? cls : (in[i] == cls ? 0 : (uint8)in[i]): the
 *                           other classes pass through (their values must fit uint8).  With a truth volume the three Dice counts
 *                           |P and T|, |P|, |T| of the filtered class (P: out == cls, T: truth == cls) are ADDED to
 *                           counts[counts_row] by integer atomics, gathered per block first.
 *
 * Invariants.  parent[i] <= i from the first store on, and every store to parent after phase 1 lowers it (atomicMin, or the root in
 * phase 3), always to a voxel of the same component.  So every find walks strictly downward and every retry of a union strictly lowers
 * the larger of its two roots: every loop has a bound known at entry (the voxel count of the tile or of the volume), and that bound
 * is in the loop condition.  A loop that exhausts it sets the `overrun` word of the workspace and leaves; the statistics row then
 * holds n_components = -1.  No block waits for another: no spin-wait, no ticket, no cooperative launch.
 * Coherence.  The L2 caches of the eight XCDs are not coherent for plain loads inside one launch.  Inside the merge launch every
 * read of parent is a device-scope atomic load and every write the atomicMin; a stale value is an earlier, larger member of the same
 * component, so it can cost a retry (the atomicMin returns what memory held) and never a wrong merge.  Phase 3 reads and writes
 * parent in place with plain accesses for the same reason; everything else relies on the launch boundary.
 *
 * vol / in, truth: D*H*W elements of the given kind, aligned to their element size.  labels: int32 [D][H][W], 4-byte aligned.  out:
 * uint8 [D][H][W]; it may be `in` itself when `in` is uint8.  stats: int64 [n_rows][4], counts: int64 [n_rows][3], both in device
 * memory and 8-byte aligned, 0 <= stats_row, counts_row < n_rows.  truth and counts may both be null (no tally); one without the
 * other is refused.  workspace: at least rpnet_cc_workspace_bytes(D, H, W) bytes, 16-byte aligned, used by one call at a time.
 * Refused with a status and an error string, before anything is launched: a null pointer, an unknown kind, a connectivity other than
 * 6 or 26, cls outside 1..255 for the uint8 output of rpnet_cc_keep_largest, a row out of range, an extent below 1 or above
 * RPNET_CC_MAX_DIM, a workspace that is too small or misaligned, `out` aliasing an `in` that is not uint8. */
size_t rpnet_cc_workspace_bytes(int D, int H, int W);
int rpnet_cc_label(const void* vol, int kind, int cls, int D, int H, int W, int connectivity, int32_t* labels, int64_t* stats,
                   int64_t stats_row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);
int rpnet_cc_keep_largest(const void* in, int kind_in, uint8_t* out, int cls, int D, int H, int W, int connectivity, const void* truth,
                          int truth_kind, int64_t* counts, int64_t counts_row, int64_t* stats, int64_t stats_row, int64_t n_rows,
                          void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_CC_ABI_H */
