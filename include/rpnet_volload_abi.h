/* C ABI of the volume-loading entry points of librpnet_hip.so: the deterministic preprocessing of FewshotVolumeReader.load_image_and_mask
 * (rpnet_amd/utils/volume_reader.py) on the device, from the payload of a file as it was uploaded (csrc/volload.hip;
 * rpnet_amd/volume_load.py): the annotated z range of the mask, one gather that composes truncate, pad to 16, the z range, centre crop
 * and symmetric pad, two exact order statistics of the cropped volume, and the percentile clip, HU clip and map to [-1, 1] of the
 * reader's `normalize`.
 *
 * A header of its own beside rpnet_abi.h and the eleven side headers before it, none of which it changes; its ledger of tests is
 * tests/volload_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_volload_abi_ledger.py.  Status codes,
 * rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h; the axis limit is that of rpnet_cc_abi.h; the element kinds of a
 * volume are those of rpnet_prep_abi.h and one more for a uint8 mask.  A library that carries these symbols says so:
 * rpnet_volload_abi_version() == RPNET_VOLLOAD_ABI_VERSION.
 *
 * Source volumes.  `kind` is RPNET_PREP_F32, RPNET_PREP_I16 or RPNET_VOLLOAD_U8.  A source has D * H * W elements, every extent 1..1024
 * (RPNET_CC_MAX_DIM), in one of two orders: RPNET_VOLLOAD_X_FASTEST, element (z, y, x) at (z * H + y) * W + x, a contiguous [D][H][W]
 * tensor; RPNET_VOLLOAD_Z_FASTEST, element (z, y, x) at z + D * (y + H * x), the payload of an NRRD file whose sizes are D H W (its first
 * axis is the fastest).
 *
 * Window (the reader's truncate_image).  From num_slice, num_y, num_x >= 1:
 *     nz = min(D, num_slice); y1 = max(0, H/2 - num_y/2), y2 = min(H, H/2 + num_y/2); x1, x2 likewise from W and num_x
 * with integer division; the window is z < nz, y1 <= y < y2, x1 <= x < x2 and must not be empty.  tH = y2 - y1, tW = x2 - x1.
 * Padded extents (pad2factor): pH = tH rounded up to a multiple of 16, pW likewise; the padding stands at the far end.
 *
 * Annotated z range.  row[0] = the first z < nz with a non-zero element in the window, row[1] = the last, row[2] = the number of
 * non-zero elements of the window, row[3] = 0; row[0] = row[1] = -1 where there is none.  Non-zero is `v != 0`: a NaN counts, as in
 * numpy.nonzero.  Integer atomics only, so two runs give the same row.
 *
 * Gather.  out is float32 [hi - lo][crop_h][crop_w] for 0 <= lo < hi <= nz.  With rh = min(crop_h, pH), cy = pH/2 - rh/2,
 * pt = (crop_h - rh)/2 (the extra row of an odd pad stands at the far end), and rw, cx, pl likewise:
 *     out[d][oy][ox] = pad_value                                 where oy < pt, oy >= pt + rh, ox < pl or ox >= pl + rw  (the crop's pad)
 *                    = pad_value                                 where py = oy - pt + cy >= tH or px = ox - pl + cx >= tW  (the pad to 16)
 *                    = (float) source(lo + d, y1 + py, x1 + px)  elsewhere.
 * The image of the reader is gathered with its pad_value, the mask with 0.  Index arithmetic only: no intermediate volume.
 *
 * Order statistics.  Of n float32 values, 1 <= n <= 2^30, the values of ranks k0 <= k1 <= n - 1 of the ascending order in which
 * -0.0 == +0.0 and every NaN stands behind +inf (numpy's sort).  The order is that of the key of the bit pattern u: a NaN has the key
 * 0xFFFFFFFF; -0.0 is taken as +0.0; a set sign bit gives ~u, a clear one u | 0x80000000.  A most-significant-digit radix selection, four
 * passes of 8 bits: a pass counts, for each of the two ranks, the digit of every key that carries the rank's prefix (histograms in LDS,
 * integer atomics; a fixed number of blocks, each striding over the array with 16 bytes per lane), and a block of 256 threads picks
 * the digit in which the rank falls.  stats[0], stats[1] = the two values as float32 (a zero is +0.0, a NaN the pattern 0x7FFFFFFF),
 * stats[2] = the number of NaNs as uint32, stats[3] = 0; they stay in device memory.
 *
 * Clip and map (the reader's `normalize`).  With a = stats[0], b = stats[1] and the weight g, every operation one float32 rounding,
 * never contracted, the division correctly rounded:
 *     d = b - a;  top = g >= 0.5 ? b - d * (1 - g) : a + d * g;  top = NaN where stats[2] != 0          (numpy's _lerp and its NaN rule)
 *     v > top -> top;  v > maximum -> maximum;  v < minimum -> minimum;  out = ((v - minimum) / denominator) * 2 - 1
 * A comparison with a NaN is false, so a NaN voxel stays one and a NaN top clips nothing.  The host passes minimum, maximum and
 * denominator = max(1, maximum - minimum) as float32 and g as numpy forms it (rpnet_amd.volume_load.percentile_rank). */
#ifndef RPNET_VOLLOAD_ABI_H
#define RPNET_VOLLOAD_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"
#include "rpnet_prep_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_VOLLOAD_ABI_VERSION 1
int rpnet_volload_abi_version(void);

/* the element kind of a mask beside RPNET_PREP_F32 (0) and RPNET_PREP_I16 (1) */
#define RPNET_VOLLOAD_U8 2

/* order of a source volume */
#define RPNET_VOLLOAD_X_FASTEST 0
#define RPNET_VOLLOAD_Z_FASTEST 1

#define RPNET_VOLLOAD_MAX_N 1073741824 /* RPNET_CC_MAX_DIM^3: the most values of a selection */
#define RPNET_VOLLOAD_SELECT_BLOCKS 1024 /* blocks of a counting pass at most; a sweep of all of them covers 1024 * 256 * 4 values */

/* The entry points launch on `stream` only: no allocation, no copy, no synchronisation, nothing read back, so every call can be captured
 * in a graph.  Every loop runs to a count fixed when it is entered; no block waits for another; the only atomics are integer ones, so
 * two runs give the same bits.
 *
 * The workspace of a selection is a 64-byte head (the prefixes and remaining ranks of the two ranks, the NaN count) and the histograms of
 * the four passes, 2 ranks * 256 digits * 4 bytes each, whatever n:
 *     rpnet_volload_select_workspace_bytes = 64 + 4 * 2 * 256 * 4.
 * The query makes no GPU call and gives 0 and an error string for n below 1 or above RPNET_VOLLOAD_MAX_N.  workspace: at least that many
 * bytes, 16-byte aligned, used by one call at a time; the first launch of a call clears it.
 *
 * Launches.  range: 3 (set the row, scan the mask 16 bytes per lane, close the row).  gather: 1, a lane writes 4 consecutive x of `out`
 * with one 16-byte store where the run is whole and aligned.  select: 9 (clear, then count and pick for each of the 4 digits).
 * normalize: 1, 16 bytes per lane, in place (out == in) or out of place.
 *
 * rpnet_volload_range      mask: D*H*W elements of `kind` in `layout`, aligned to the element.  row: 4 int32, 16-byte aligned.
 * rpnet_volload_gather     src as above; out: (hi - lo) * crop_h * crop_w float32, 4-byte aligned; crop_h, crop_w 1..RPNET_CC_MAX_DIM.
 * rpnet_volload_select     x: n float32, 4-byte aligned.  stats: 4 words, 16-byte aligned.  0 <= k0 <= k1 <= n - 1.
 * rpnet_volload_normalize  in, out: n float32, 4-byte aligned, the same address or disjoint.  stats: as select leaves it.
 *   minimum <= maximum, denominator >= 1, 0 <= g < 1, none a NaN.
 * Refused with a status and an error string, before anything is launched: a null pointer, an unknown kind or layout, an extent below 1
 * or above RPNET_CC_MAX_DIM, num_slice, num_y or num_x below 1 or an empty window, lo and hi outside 0 <= lo < hi <= nz, n out of range,
 * ranks out of order or range, a workspace that is too small or misaligned, a misaligned pointer, out partly overlapping in, bounds or
 * a weight outside their ranges. */
size_t rpnet_volload_select_workspace_bytes(size_t n);
int rpnet_volload_range(const void* mask, int kind, int layout, int D, int H, int W, int num_slice, int num_y, int num_x, int32_t* row,
                        rpnet_stream_t stream);
int rpnet_volload_gather(const void* src, int kind, int layout, int D, int H, int W, int num_slice, int num_y, int num_x, int lo, int hi,
                         int crop_h, int crop_w, float pad_value, float* out, rpnet_stream_t stream);
int rpnet_volload_select(const float* x, size_t n, size_t k0, size_t k1, void* stats, void* workspace, size_t workspace_bytes,
                         rpnet_stream_t stream);
int rpnet_volload_normalize(const float* in, float* out, size_t n, const void* stats, float g, float minimum, float maximum,
                            float denominator, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_VOLLOAD_ABI_H */
