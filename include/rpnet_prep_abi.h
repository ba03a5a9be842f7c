/* C ABI of the body-mask preprocessing entry points of librpnet_hip.so: the per-slice threshold (fixed or Otsu) of a raw CT volume, the
 * connected region of a seed pixel per slice, and the pass that masks the volume and finds the bounding box of what is left
 * (csrc/prep.hip; rpnet_amd/preprocess.py, tools/preprocess_volumes.py).  With rpnet_morph_apply (per_slice) and rpnet_ccpost_fill_holes
 * (slice mode) between them they are the chain that makes `<pid>_clean.nrrd` from a raw volume.
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h, rpnet_guard_abi.h, rpnet_surface_abi.h, rpnet_cc_abi.h,
 * rpnet_surface_spacing_abi.h, rpnet_ccpost_abi.h and rpnet_morph_abi.h, none of which it changes; its ledger of tests is
 * tests/prep_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_prep_abi_ledger.py.  Status codes, rpnet_stream_t
 * and rpnet_last_error_string() are those of rpnet_abi.h; the axis limit and the `overrun` word are those of rpnet_cc_abi.h.  A library
 * that carries these symbols says so: rpnet_prep_abi_version() == RPNET_PREP_ABI_VERSION.
 *
 * An image is [D][H][W] float32 or int16; a mask is uint8 [D][H][W].  Every z slice is its own 2D image in the first two entry points.
 * fl(.) is one IEEE-754 binary64 rounding; csrc/prep.hip is built without FMA contraction.
 *
 * Threshold, fixed mode.  Foreground is `(double)v > t`.  NaN is background.
 *
 * Threshold, Otsu mode.
 *  1. `lo` and `hi` are the smallest and largest finite value of the slice.  They are compared by value and converted to double exactly.
 *  2. Non-finite voxels take no part and are background.
 *  3. If the slice has no finite voxel, or `hi == lo`, the mask of that slice is empty and `k* = -1`.
 *  4. With `n = 128` bins, compute `scale = fl(128.0 / fl(hi - lo))`.
 *  5. Bin each voxel with `b(v) = min(127, (int)fl(fl((double)v - lo) * scale))`.
 *  6. `c_b` are the counts and `N` is their sum.  `w(k)` is the sum of `c_b` for `b <= k`.  `m(k)` is the sum of `b * c_b` for `b <= k`.
 *     All four are int64.
 *  7. For `k` = 0..126 with `0 < w(k) < N`:
 *     - `num = (double)(m(127) * w(k) - m(k) * N)`.  This is an exact integer below 2^53 for a slice of at most 1024^2.
 *     - `val(k) = fl(fl(num * num) / fl((double)w(k) * (double)(N - w(k))))`.
 *  8. `k*` is the first `k` with the largest `val`.
 *  9. Foreground is `b(v) > k*`.
 * 10. The reported threshold is `fl(lo + fl((k* + 1) * fl(fl(hi - lo) / 128.0)))`.
 * This gives the same mask as `1 - sitk.OtsuThreshold(img)` whenever ITK's calculator picks the same bin.  Parity with ITK's own binning
 * and return value is not claimed.
 * The rows of a slice: int64 {n_finite, k*, n_foreground, 0} and float64 {lo, hi, threshold}.  A slice without a finite voxel reports
 * lo = hi = 0 (n_finite = 0 says so); a zero of either sign is reported as +0.  In fixed mode k* = -1 and the threshold is t; with
 * hi == lo in Otsu mode the formula of step 10 gives lo.
 *
 * Seeded component.  The object of slice z is `mask == cls`; two object pixels of a slice are neighbours when they share an edge
 * (connectivity 4) or an edge or a corner (8); there is no link across z.  If the seed pixel (y, x) of the slice belongs to the object,
 * the output keeps cls on the component of the seed and every other object pixel becomes 0; if it does not, the whole slice loses the
 * class.  Other values pass through.  The row of a slice: int64 {seed_hit, voxels_before, voxels_kept, n_components}; n_components is
 * -1 when a bounded loop of the labelling ran out of its bound (the `overrun` word of the workspace, RPNET_CC_OVERRUN_OFFSET).
 *
 * Mask and box.  out[i] = mask[i] ? img[i] : fill, in the image's own kind.  A voxel is kept when `mask[i] && (double)img[i] >
 * (double)fill` (NaN is not kept): the reference takes its box over `processed_image > -1024`.  The row: int64 {zmin, zmax, ymin, ymax,
 * xmin, xmax, n_kept, n_mask}, the extents inclusive and all six -1 when nothing is kept; n_mask counts `mask != 0`.
 *
 * Everything is integer work or separately rounded fp64 in a fixed order, with integer atomics only: two runs give the same bits. */
#ifndef RPNET_PREP_ABI_H
#define RPNET_PREP_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_PREP_ABI_VERSION 1
int rpnet_prep_abi_version(void);

/* element kinds of an image */
#define RPNET_PREP_F32 0
#define RPNET_PREP_I16 1

/* mode of rpnet_prep_threshold */
#define RPNET_PREP_FIXED 0
#define RPNET_PREP_OTSU 1
#define RPNET_PREP_OTSU_BINS 128

/* columns of the tables */
#define RPNET_PREP_THRESHOLD_ROW 4  /* int64 per slice: n_finite, k*, n_foreground, 0 */
#define RPNET_PREP_THRESHOLD_FROW 3 /* float64 per slice: lo, hi, threshold */
#define RPNET_PREP_SEED_ROW 4       /* int64 per slice: seed_hit, voxels_before, voxels_kept, n_components */
#define RPNET_PREP_BBOX_ROW 8       /* int64: zmin, zmax, ymin, ymax, xmin, xmax, n_kept, n_mask */

/* Every entry point launches on `stream` only: no allocation, no synchronisation, nothing read back, so a call can be captured in a
 * graph; the words of the workspace a call reads are cleared by its own first launch.  Every loop carries its bound in its condition;
 * no block waits for another.  Every *_workspace_bytes query makes no GPU call and gives 0 and an error string for an extent below 1 or
 * above RPNET_CC_MAX_DIM.  workspace: at least that many bytes, 16-byte aligned, used by one call at a time.
 *
 * rpnet_prep_threshold  (a 64-byte head and 136 uint32 per slice: 128 bins, min, max, n_foreground, n_finite, k*, 3 spare)
 *   1. clear; 2. per-slice min, max and finite count: the values through an order-preserving uint32 encoding, reduced per block in LDS,
 *   then one integer atomicMin / atomicMax / atomicAdd per block; 3. (Otsu) the 128-bin histogram in LDS per block, then integer
 *   atomicAdd of the bins a block met; 4. the mask: every block redoes the scan of steps 6 to 8 from its slice's histogram (one thread
 *   per k, then a first-maximum walk of 127 steps) and writes 16 voxels per lane, one 16-byte store where the address allows it;
 *   5. one thread per slice writes the two rows.
 *   img: D*H*W elements of `kind`, aligned to the element.  mask: uint8, must not overlap img.  rows_i: int64 [D][4], rows_f: float64
 *   [D][3], 8-byte aligned.  t is read in fixed mode only and must not be NaN there.
 * rpnet_prep_seeded_component  (a 64-byte head, two int32 volumes and 4 uint32 per slice)
 *   1. clear; 2. local labelling, 3. seam merge, 4. flatten: the phases of csrc/cc_phases.h without a z link; 5. select and write:
 *   out = parent[i] == parent[seed of the slice] ? cls : (in == cls ? 0 : in), 16 voxels per lane, the counts per block first;
 *   6. one thread per slice writes the row.
 *   in, out: uint8; out may be `in` itself, any other overlap is refused.  0 <= seed_y < H, 0 <= seed_x < W.  stats: int64 [D][4].
 * rpnet_prep_mask_bbox  (a 64-byte head)
 *   1. clear; 2. mask, write and reduce: 16 voxels per lane with 16-byte loads and stores where the addresses allow it, extents and
 *   counts per block in LDS, then one integer atomicMin / atomicMax / atomicAdd per block; 3. one launch writes rows[row].
 *   out: the image's kind; it may be `img` itself, any other overlap with img or mask is refused.  fill must be a value of the image's
 *   kind (-1024 is).  rows: int64 [n_rows][8], 0 <= row < n_rows.
 * Refused with a status and an error string, before anything is launched: a null pointer, an unknown kind or mode, an extent below 1 or
 * above RPNET_CC_MAX_DIM, cls outside 1..255, a seed outside the slice, a connectivity other than 4 or 8, a row out of range, a NaN
 * threshold, a fill the kind cannot hold, a workspace that is too small or misaligned, a misaligned image or table, an overlap. */
size_t rpnet_prep_threshold_workspace_bytes(int D, int H, int W);
int rpnet_prep_threshold(const void* img, int kind, uint8_t* mask, int D, int H, int W, int mode, double t, int64_t* rows_i, double* rows_f,
                         void* workspace, size_t workspace_bytes, rpnet_stream_t stream);
size_t rpnet_prep_seeded_component_workspace_bytes(int D, int H, int W);
int rpnet_prep_seeded_component(const uint8_t* in, uint8_t* out, int cls, int D, int H, int W, int seed_y, int seed_x, int connectivity,
                                int64_t* stats, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);
size_t rpnet_prep_mask_bbox_workspace_bytes(int D, int H, int W);
int rpnet_prep_mask_bbox(const void* img, int kind, const uint8_t* mask, void* out, double fill, int D, int H, int W, int64_t* rows,
                         int64_t row, int64_t n_rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_PREP_ABI_H */
