/* C ABI of the region-statistics entry points of librpnet_hip.so: per label of a segmented volume, in one pass over the label volume
 * and an image, the exact integer geometry (count, bounding box, first and second coordinate moments) and bit-reproducible float64
 * intensity sums (csrc/regions.hip; rpnet_amd/regions.py).
 *
 * A header of its own beside rpnet_abi.h and the fourteen side headers before it, none of which it changes; its ledger of tests is
 * tests/regions_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_regions_abi_ledger.py.  Status codes,
 * rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h; the label kinds and the largest extent are those of
 * rpnet_cc_abi.h; the image kinds are RPNET_PREP_F32 and RPNET_PREP_I16 of rpnet_prep_abi.h, as in the resample and smooth headers.  A
 * library that carries these symbols says so: rpnet_region_abi_version() == RPNET_REGION_ABI_VERSION.
 *
 * Definitions.  A label volume [D][H][W] of one label kind and, optionally, an image [D][H][W] of one image kind; voxel (z, y, x) has
 * the linear index i = z*H*W + y*W + x.  Labels lo .. L-1 are tallied, lo in {0, 1}, 1 <= L <= RPNET_REGION_MAX_LABELS; with lo = 1 the
 * row of label 0 is written as an empty row.  A voxel whose value is not an integer in 0 .. L-1 (float32 labels: value == (float)l for
 * no such l; a negative value, a non-integer and a NaN among them) is counted in the n_outside word of the workspace and enters no row.
 *
 * rows_i[row], int64 [L][RPNET_REGION_IROW], every entry exact (integer atomics only, so the order in which blocks run cannot show):
 *   0        n, the voxels of the label
 *   1..3     min z, y, x                       an empty label holds D, H, W
 *   4..6     max z, y, x                       an empty label holds -1
 *   7..9     sum z, sum y, sum x
 *   10..12   sum z*z, sum y*y, sum x*x
 *   13..15   sum z*y, sum z*x, sum y*x
 *   16       n_finite, the voxels of the label whose image value is finite
 *   17, 18   the smallest and the largest key over those voxels: the order-preserving key of the float32 pattern of
 *            rpnet_volload_abi.h (-0.0 taken as +0.0; a set sign bit gives ~u, a clear one u | 0x80000000); an int16 value enters as
 *            (float)v, which is exact.  An empty label holds 0xFFFFFFFF and 0
 *   19       0
 * With extents up to RPNET_CC_MAX_DIM = 1024 every sum is below 2^50 (2^30 voxels x 2^20).  Without an image columns 16..18 are those
 * of an empty row.
 *
 * rows_f[row], float64 [L][RPNET_REGION_FROW]: S1 = SUM (double)v and S2 = SUM (double)v * (double)v over the finite voxels of the
 * label (the product of two float32 values is exact in float64: only the additions round, each once, never contracted).  Non-finite
 * voxels enter neither sum nor the keys; n - n_finite counts them.  Without an image, and for a label below lo, both are +0.0.
 *
 * SUM, the order of the additions, is part of this ABI, so that a numpy restatement gives the same bits (tests/regions_cases.py):
 *   - the volume in linear order is cut into chunks of RPNET_REGION_CHUNK = 4096 voxels; lane t (0..255) of a chunk owns its voxels
 *     16 t .. 16 t + 15; positions beyond the end of the volume hold nothing;
 *   - for a label l, lane t forms a_t: from +0.0 it adds the terms of its voxels of label l in ascending index (+0.0 where it has none);
 *   - the value of the chunk is the stride-halving tree over the 256 a_t: a[t] = a[t] + a[t + s] for t < s, s = 128, 64, ..., 1;
 *   - G = min(number of chunks, RPNET_REGION_MAX_BLOCKS) blocks run; block b takes the chunks b, b + G, b + 2G, ... and, from +0.0,
 *     adds their values in that ascending order into P_b[l].  Every partial starts at +0.0 and no chunk value is -0.0, so a chunk
 *     without the label may be skipped or added as +0.0 with the same bits;
 *   - a second launch, one block of 256 threads per label, folds P_0 .. P_{G-1} of its label by the SUM of rpnet_fusion_abi.h: thread t
 *     adds P_t, P_{t+256}, ... in ascending order from 0.0, then the same tree runs.  That launch writes rows_f and, from the integer
 *     accumulators of the workspace, rows_i.
 *
 * Workspace (bytes, n = D*H*W, G = min((n + 4095) / 4096, 1024)):
 *     head 64 | accumulators int64 [L][20] | partials float64 [G][L][2]
 *   rpnet_region_workspace_bytes = 64 + 160 * L + 16 * G * L
 * The head holds n_outside, an int64, at byte RPNET_REGION_OUTSIDE_OFFSET.  One memset on `stream` clears the head and the accumulators;
 * zero is the identity of every accumulator because the extrema are kept as maxima of an encoding: column 1..3 as 1024 - min,
 * 4..6 as max + 1, 17 as 0xFFFFFFFF - key.  The second launch decodes them.  The partials need no clearing: every block writes its own. */
#ifndef RPNET_REGION_ABI_H
#define RPNET_REGION_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"
#include "rpnet_prep_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_REGION_ABI_VERSION 1
int rpnet_region_abi_version(void);

#define RPNET_REGION_MAX_LABELS 256
#define RPNET_REGION_IROW 20
#define RPNET_REGION_FROW 2
#define RPNET_REGION_CHUNK 4096 /* 256 lanes x 16 voxels */
#define RPNET_REGION_MAX_BLOCKS 1024
#define RPNET_REGION_HEAD_BYTES 64
#define RPNET_REGION_OUTSIDE_OFFSET 0 /* int64 n_outside in the head of the workspace */

/* The entry point launches on `stream` only: no allocation, no synchronisation, nothing read back, so the call can be captured in a
 * graph.  Integer atomics only, no floating-point atomic anywhere; no block waits for another, no cooperative launch; the launch
 * boundary is the only synchronisation between the pass and the fold; every loop runs to a count fixed when it is entered.  Two runs
 * give the same bits.
 *
 * rpnet_region_workspace_bytes  the formula above; no GPU call; 0 and an error string for an extent outside 1..RPNET_CC_MAX_DIM or L
 *                         outside 1..RPNET_REGION_MAX_LABELS.
 * rpnet_region_stats      one memset, the pass (G blocks of 256 lanes; a lane reads its 16 voxels with 16-byte accesses where it is
 *                         whole and aligned, element by element otherwise) and the fold.  It WRITES the L rows of `row`; it does not
 *                         add to them.
 *
 * labels: D*H*W elements of label_kind (RPNET_CC_U8 / I32 / I64 / F32), aligned to the element.  image: null, or D*H*W elements of
 * image_kind (RPNET_PREP_F32 / RPNET_PREP_I16), aligned to the element; with a null image image_kind is ignored and rows_f may be null.
 * rows_i int64 [n_rows][L][20], rows_f float64 [n_rows][L][2]: device memory, 8-byte aligned, 0 <= row < n_rows.  workspace: at least
 * rpnet_region_workspace_bytes(D, H, W, L) bytes, 16-byte aligned, used by one call at a time.
 * Refused with a status and an error string, before anything is launched: a null labels, rows_i or workspace; rows_f null while image
 * is not; an unknown kind; lo outside {0, 1}, L outside 1..256, lo >= L unless L == 1 and lo == 1 (which writes one empty row); an
 * extent outside 1..1024; a row out of range; a workspace that is too small or not 16-byte aligned; a pointer not aligned to its
 * element (8 bytes for the tables). */
size_t rpnet_region_workspace_bytes(int D, int H, int W, int L);
int rpnet_region_stats(const void* labels, int label_kind, const void* image, int image_kind, int D, int H, int W, int lo, int L,
                       int64_t* rows_i, double* rows_f, int64_t row, int64_t n_rows, void* workspace, size_t workspace_bytes,
                       rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_REGION_ABI_H */
