/* C ABI of the per-component statistics of librpnet_hip.so: the dense renumbering of the sparse component labels of rpnet_cc_label and,
 * per component, in one pass over the renumbered volume, an image and a second volume, the exact integer geometry, exact integer
 * intensity sums of the quantised image and the overlap with a class of the second volume (csrc/compstat.hip;
 * rpnet_amd/component_stats.py).
 *
 * A header of its own beside rpnet_abi.h and the fifteen side headers before it, none of which it changes; its ledger of tests is
 * tests/compstat_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_compstat_abi_ledger.py.  Status codes,
 * rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h; the label kinds and the largest extent are those of
 * rpnet_cc_abi.h; the image kinds are RPNET_PREP_F32 and RPNET_PREP_I16 of rpnet_prep_abi.h.  A library that carries these symbols says
 * so: rpnet_compstat_abi_version() == RPNET_COMPSTAT_ABI_VERSION.
 *
 * Definitions.  A volume [D][H][W]; voxel (z, y, x) has the linear index i = z*H*W + y*W + x, n = D*H*W.
 *
 * labels, int32 [D][H][W], are those of rpnet_cc_label: 0, or 1 + the smallest linear index of the voxel's component.  Voxel i is a
 * ROOT iff labels[i] == i + 1; the id of its component is 1 + the number of roots below i, so the ids 1 .. C number the components by
 * their first voxel in z-major order, which is scipy.ndimage.label's own numbering.  dense[i] is 0 where labels[i] == 0, the id of the
 * root labels[i] - 1 where that voxel is a root, and 0 where it is not (labels[i] outside 1..n, or labels[labels[i] - 1] != labels[i]):
 * such a voxel is counted in the `invalid` word of the head and nothing is read out of bounds for it.
 *
 * rows[row], int64 [max_components][RPNET_COMPSTAT_ROW], row k - 1 for the id k; every entry exact (integer atomics only, so the order
 * in which blocks and atomics run cannot show):
 *   0..15    n | min z y x | max z y x | sum z y x | sum zz yy xx | sum zy zx yx: columns 0..15 of rpnet_region_abi.h; an empty row
 *            holds n = 0, min = D, H, W, max = -1
 *   16       n_summed, the voxels of the component whose image value is finite and representable (below)
 *   17, 18   the smallest and the largest order-preserving key of the float32 pattern (rpnet_volload_abi.h; -0.0 taken as +0.0; an
 *            int16 value enters as (float)v) over those voxels; an empty row holds 0xFFFFFFFF and 0
 *   19       S1 = SUM k
 *   20, 21   SUM (k*k & 0xFFFFFFFF) and SUM (k*k >> 32): S2 = SUM k*k = [20] + ([21] << 32), exact as an unbounded integer
 *   22       n_overlap, the voxels of the component where other == other_cls; 0 without `other`
 *   23       the linear index of the first voxel; -1 in an empty row
 * k = rint((double)v * 2^q), ties to even, q = scale_log2 in 0..30; the product is exact, so k is the one rounding.  A value is
 * representable when it is finite and |k| < 2^31.  Every other voxel is counted in n - n_summed and enters no sum and no key.  The
 * quantised value k / 2^q differs from v by at most 2^-(q+1), so the mean the host derives lies within 2^-(q+1) of the float64 mean of
 * the same voxels and the standard deviation within 2^-(q+1) of theirs (the root of a mean square is a norm: the triangle inequality).
 * An int16 value enters as itself at q = 0.  With extents up to 1024 every column is below 2^62 in magnitude.
 * Every row of rows[row] is WRITTEN: the ids above C hold the empty row.  Voxels whose id exceeds max_components enter no row and are
 * counted in n_beyond; a dense value outside 0..C enters no row and is counted in the table's `invalid` word.  Without an image
 * columns 16..21 are those of an empty row.
 *
 * Workspace (bytes, n = D*H*W, nc = (n + 4095) / 4096 chunks):
 *     head 64 | chunk counts int32 [nc rounded up to 4] | rank int32 [n]
 *   rpnet_compstat_workspace_bytes = 64 + 4 * ((nc + 3) / 4 * 4) + 4 * n
 * (the accumulators are the rows themselves, so max_components is checked and does not enter).  The head holds four int64 words:
 * n_components C at byte RPNET_COMPSTAT_COUNT_OFFSET and the `invalid` count of rpnet_compstat_rank at RPNET_COMPSTAT_INVALID_OFFSET,
 * both written by rpnet_compstat_rank; n_beyond at RPNET_COMPSTAT_BEYOND_OFFSET and the `invalid` count of rpnet_compstat_table at
 * RPNET_COMPSTAT_TABLE_INVALID_OFFSET, both written by rpnet_compstat_table, which READS C from the head: it follows a
 * rpnet_compstat_rank call on the same workspace (or a head the caller filled). */
#ifndef RPNET_COMPSTAT_ABI_H
#define RPNET_COMPSTAT_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"
#include "rpnet_prep_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_COMPSTAT_ABI_VERSION 1
int rpnet_compstat_abi_version(void);

#define RPNET_COMPSTAT_MAX_COMPONENTS 65536
#define RPNET_COMPSTAT_ROW 24
#define RPNET_COMPSTAT_STATS_ROW 4   /* int64: n_components, invalid, 0, 0 */
#define RPNET_COMPSTAT_CHUNK 4096    /* 256 lanes x 16 voxels: the cut of RPNET_REGION_CHUNK */
#define RPNET_COMPSTAT_SCAN_THREADS 256
#define RPNET_COMPSTAT_SLOTS 128     /* ids a block gathers in LDS per chunk (below) */
#define RPNET_COMPSTAT_MAX_BLOCKS 2048
#define RPNET_COMPSTAT_MAX_SCALE_LOG2 30
#define RPNET_COMPSTAT_HEAD_BYTES 64
#define RPNET_COMPSTAT_COUNT_OFFSET 0
#define RPNET_COMPSTAT_INVALID_OFFSET 8
#define RPNET_COMPSTAT_BEYOND_OFFSET 16
#define RPNET_COMPSTAT_TABLE_INVALID_OFFSET 24

/* Every entry point launches on `stream` only: no allocation, no synchronisation, nothing read back, so a call can be captured in a
 * graph.  Integer atomics only, no floating-point atomic anywhere; no block waits for another, no cooperative launch; the launch
 * boundary is the only synchronisation (the L2 caches of the XCDs are not coherent inside a launch: nothing is gathered in the launch
 * that writes it); every loop runs to a count fixed when it is entered.  Two runs give the same bits.
 *
 * rpnet_compstat_workspace_bytes  the formula above; no GPU call; 0 and an error string for an extent outside 1..RPNET_CC_MAX_DIM or
 *                        max_components outside 1..RPNET_COMPSTAT_MAX_COMPONENTS.
 * rpnet_compstat_rank    a fixed-order exclusive scan: one memset of the head, then
 *                        1. count: one block of 256 lanes per chunk of 4096 voxels (lane t owns the voxels 16 t .. 16 t + 15 of the
 *                           chunk) counts its roots into the chunk counts;
 *                        2. scan: ONE block of RPNET_COMPSTAT_SCAN_THREADS threads turns the counts into exclusive offsets, tile of
 *                           256 chunks by tile with a running carry, and writes C into the head;
 *                        3. roots: a block per chunk; every root writes its id into rank[i];
 *                        4. gather: dense[i] = rank[labels[i] - 1], bound-checked and root-checked first (the roots and the labels
 *                           were written before this launch began);
 *                        5. one thread writes stats[stats_row] = {C, invalid, 0, 0} where stats is not null.
 *                        dense may not alias labels.
 * rpnet_compstat_table   one memset of rows[row] and of the table's two head words, the pass and a decode launch.  The pass: G =
 *                        min(nc, RPNET_COMPSTAT_MAX_BLOCKS) blocks of 256 lanes walk the chunks b, b + G, ...; a lane reads its 16
 *                        voxels with 16-byte accesses where it is whole and aligned.  A wave that holds one id in all its voxels
 *                        (the inside of an organ) folds its 1024 voxels by wave reductions and adds once; elsewhere a lane folds its
 *                        runs of equal ids in registers.  Both add into an LDS table of RPNET_COMPSTAT_SLOTS = 128 slots (an id and 24
 *                        int64 accumulators: 25096 bytes of LDS per block) by LDS integer atomics; the slot of an id is found by at
 *                        most 8 linear probes from a multiplicative hash.  The slot count follows from the occupancy the registers
 *                        allow, not from the 160 KiB alone: the compiler gives the pass 104 to 112 VGPRs and no scratch, which is
 *                        four waves per SIMD, four blocks per compute unit, so a block may hold 40 KiB of LDS; the hash masks with
 *                        the slot count, so it is a power of two, and 128 is the largest that fits (256 slots are 49 KiB: three
 *                        blocks).  A build forced to 80 VGPRs reaches six waves and spills 88 to 96 bytes per lane; neither that
 *                        build nor a counter of this one has been run.
 *                        At the end of a chunk every used slot is flushed with one global atomic per column that is not the
 *                        identity, so a volume of one id costs one row's atomics per chunk, not per voxel.  A run that finds no slot
 *                        within its probes goes to global atomics directly.  The extrema are kept as maxima of an encoding of which
 *                        0 is the identity (columns 1..3 as 1024 - min, 4..6 as max + 1, 17 as 0xFFFFFFFF - key, 23 as 2^30 - index),
 *                        so the memset clears the rows; the decode launch rewrites those columns in place.
 *
 * labels, dense: int32 [D][H][W], 4-byte aligned.  image: null, or D*H*W elements of image_kind (RPNET_PREP_F32 / RPNET_PREP_I16),
 * aligned to the element; with a null image image_kind and scale_log2 are ignored.  other: null, or D*H*W elements of other_kind
 * (RPNET_CC_U8 / I32 / I64 / F32; a voxel overlaps when value == other_cls, fp32: == (float)other_cls), aligned to the element.  stats
 * int64 [n_rows][4] or null, rows int64 [n_rows][max_components][24]: device memory, 8-byte aligned, 0 <= row < n_rows.  workspace: at
 * least rpnet_compstat_workspace_bytes bytes, 16-byte aligned, used by one call at a time.
 * Refused with a status and an error string, before anything is launched: a null labels, dense, rows or workspace; dense == labels; an
 * unknown kind; scale_log2 outside 0..30 with an image; max_components outside 1..65536; an extent outside 1..1024; a row out of range;
 * a workspace that is too small or not 16-byte aligned; a pointer not aligned to its element (8 bytes for the tables). */
size_t rpnet_compstat_workspace_bytes(int D, int H, int W, int max_components);
int rpnet_compstat_rank(const int32_t* labels, int D, int H, int W, int32_t* dense, int64_t* stats, int64_t stats_row, int64_t n_rows,
                        void* workspace, size_t workspace_bytes, rpnet_stream_t stream);
int rpnet_compstat_table(const int32_t* dense, const void* image, int image_kind, int scale_log2, const void* other, int other_kind,
                         int other_cls, int D, int H, int W, int max_components, int64_t* rows, int64_t row, int64_t n_rows, void* workspace,
                         size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_COMPSTAT_ABI_H */
