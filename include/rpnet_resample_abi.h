/* C ABI of the resampling entry points of librpnet_hip.so: a [D][H][W] image or label map taken to a grid of another shape, trilinear or
 * nearest neighbour (csrc/resample.hip; rpnet_amd/resample.py, tools/preprocess_volumes.py --resample).  It is the `resample(image,
 * spacing, new_spacing)` stage of the reference's utils/preprocess_abd_110.py, called there on the image and on every structure and
 * followed by `> 0.5` on the structures.  The reference imports that function from a module it does not ship, so the definition below is
 * this project's own, pinned to scipy.ndimage.zoom by tests/test_host_resample.py; parity with the missing module is not claimed.
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h, rpnet_guard_abi.h, rpnet_surface_abi.h, rpnet_cc_abi.h,
 * rpnet_surface_spacing_abi.h, rpnet_ccpost_abi.h, rpnet_morph_abi.h and rpnet_prep_abi.h, none of which it changes; its ledger of tests is
 * tests/resample_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_resample_abi_ledger.py.  Status codes,
 * rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h; the axis limit is that of rpnet_cc_abi.h; the element kinds of an
 * image are those of rpnet_prep_abi.h.  A library that carries these symbols says so: rpnet_resample_abi_version() ==
 * RPNET_RESAMPLE_ABI_VERSION.
 *
 * An image is contiguous [D][H][W] float32 or int16, the RPNET_PREP_F32 / RPNET_PREP_I16 kinds.  A label map is uint8.  Every axis
 * length, input and output, is 1..1024 (RPNET_CC_MAX_DIM).  fl(.) is one float64 rounding; csrc/resample.hip is built with
 * -ffp-contract=off, as prep.hip and surface_spacing.hip are built.
 *
 * Coordinates.  For output index `o` on an axis of input length `n` and output length `m`:
 *  - align = CORNER: `c = fl((double)(o * (n - 1)) / (double)(m - 1))`, and `c = 0` when `m == 1`.  This is scipy's
 *    `zoom(grid_mode=False)`.
 *  - align = CENTER: `c = fl(fl((double)((2o + 1) * n) / (double)(2m)) - 0.5)`, clamped to `[0, n - 1]`.  This is `grid_mode=True,
 *    mode='nearest'` and torch's `align_corners=False`.
 *  - The integer products are exact.
 *  - `i0 = min((int)floor(c), n - 1)`, `i1 = min(i0 + 1, n - 1)`, `t = c - i0`.
 * Linear.
 *  - `lerp(a, b, t) = a` when `t == 0`.  A tap of weight zero is not used, so an identity resample is bit-exact and a non-finite
 *    neighbour does not leak.
 *  - Otherwise `lerp(a, b, t) = fl(a + fl(t * fl(b - a)))`.
 *  - The order is four lerps along x, then two along y, then one along z, on the voxels widened to float64.
 *  - The result takes one conversion to the output kind.  float32 rounds to nearest.  int16 rounds half to even and saturates to
 *    [-32768, 32767].
 * Nearest.  `i = clamp((int)floor(fl(c + 0.5)), 0, n - 1)` per axis.
 * Labels, mode NEAREST.  The label at the nearest voxel.
 * Labels, mode LINEAR, one class `cls` per call.  Apply the linear rule above to the indicator `(v == cls)`.  The voxel is of the class
 * when the result is `> 0.5`; exactly 0.5 is not.  This is the reference's `resample(mask) > 0.5`.
 *  - With `merge = 0`, the output is `cls` or 0.
 *  - With `merge = 1`, the output takes `cls` only where it currently holds 0.  This matches the morphology's "gained voxels take the
 *    class only over 0".
 * Statistics row (labels only): int64 {voxels_in, voxels_out, out_voxels_total, 0} for the class: the input voxels equal to `cls`, the
 * output voxels that hold `cls` when the call has finished, and Do * Ho * Wo.  It is formed with integer atomics only, so two runs give
 * the same bits.
 * Not done.  No anti-aliasing filter when shrinking; scipy has none either.  No oblique grids.  No spline order above 1. */
#ifndef RPNET_RESAMPLE_ABI_H
#define RPNET_RESAMPLE_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"
#include "rpnet_prep_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_RESAMPLE_ABI_VERSION 1
int rpnet_resample_abi_version(void);

/* align */
#define RPNET_RESAMPLE_CORNER 0
#define RPNET_RESAMPLE_CENTER 1

/* order of rpnet_resample_image, mode of rpnet_resample_labels */
#define RPNET_RESAMPLE_NEAREST 0
#define RPNET_RESAMPLE_LINEAR 1

#define RPNET_RESAMPLE_STATS_ROW 4 /* int64: voxels_in, voxels_out, out_voxels_total, 0 */

/* Both entry points launch on `stream` only: no allocation, no copy, no synchronisation, nothing read back, so a call can be captured in
 * a graph.  Every loop runs to a count fixed when it is entered; no block waits for another.
 *
 * The workspace is a 64-byte head (the two counters of the statistics row) and one 16-byte entry {int32 i0, int32 i1, float64 t} per
 * output index of each axis, z then y then x; under NEAREST i0 is the nearest index and i1 and t are 0:
 *     rpnet_resample_workspace_bytes = 64 + 16 * (Do + Ho + Wo).
 * The query makes no GPU call and gives 0 and an error string for an extent below 1 or above RPNET_CC_MAX_DIM.  workspace: at least that
 * many bytes, 16-byte aligned, used by one call at a time.
 *
 * The launches of a call: 1. one small launch clears the head and writes the three tables; 2. (labels with a statistics row) a count of
 * the input voxels equal to cls, 16 per lane, one integer atomic per block; 3. the gather: a lane owns a run of 16 bytes of consecutive
 * output x positions of one output row (4 float32, 8 int16, 16 uint8), reads its taps through the tables and writes the run with one
 * 16-byte store where the run is whole and its address 16-byte aligned (decided per lane) and element by element otherwise; the count of
 * the output per block, then one integer atomic; 4. (statistics) one launch writes stats[row].
 *
 * rpnet_resample_image   in: Di*Hi*Wi elements of `kind`, out: Do*Ho*Wo of the same kind, both aligned to the element; they must not
 *   overlap.  order: NEAREST copies the voxel's bits; LINEAR is the rule above.
 * rpnet_resample_labels  in, out: uint8, must not overlap.  cls: 1..255 under LINEAR; under NEAREST it only names the class the
 *   statistics row counts, 0..255.  merge is read under LINEAR only, where merge = 1 also reads `out`.  stats: int64 [rows][4], 8-byte
 *   aligned, 0 <= row < rows; or null, and then no statistics are formed and row and rows are not read.
 * Refused with a status and an error string, before anything is launched: a null pointer, an unknown kind, align, order, mode or merge, an
 * extent below 1 or above RPNET_CC_MAX_DIM, a class outside its range, a row out of range, a workspace that is too small or misaligned,
 * a misaligned volume or table, an overlap. */
size_t rpnet_resample_workspace_bytes(int Di, int Hi, int Wi, int Do, int Ho, int Wo);
int rpnet_resample_image(const void* in, int kind, int Di, int Hi, int Wi, void* out, int Do, int Ho, int Wo, int align, int order,
                         void* workspace, size_t workspace_bytes, rpnet_stream_t stream);
int rpnet_resample_labels(const uint8_t* in, int Di, int Hi, int Wi, uint8_t* out, int Do, int Ho, int Wo, int cls, int align, int mode,
                          int merge, int64_t* stats, int64_t row, int64_t rows, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_RESAMPLE_ABI_H */
