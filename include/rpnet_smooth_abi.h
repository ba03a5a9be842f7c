/* C ABI of the smoothing entry point of librpnet_hip.so: a separable Gaussian filter of a [D][H][W] float32 or int16 volume
 * (csrc/smooth.hip; rpnet_amd/smooth.py; the `antialias` option of rpnet_amd/resample.py and tools/preprocess_volumes.py --antialias).
 * It is the device form of scipy.ndimage.gaussian_filter, to which tests/test_host_smooth.py pins the definition below, and the
 * prefilter a shrinking resample needs: point samples of the trilinear interpolant fold every frequency above the new Nyquist limit into
 * the image.
 *
 * A header of its own beside rpnet_abi.h, rpnet_eval_abi.h, rpnet_optim_abi.h, rpnet_guard_abi.h, rpnet_surface_abi.h, rpnet_cc_abi.h,
 * rpnet_surface_spacing_abi.h, rpnet_ccpost_abi.h, rpnet_morph_abi.h, rpnet_prep_abi.h and rpnet_resample_abi.h, none of which it changes;
 * its ledger of tests is tests/smooth_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_smooth_abi_ledger.py.
 * Status codes, rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h; the axis limit is that of rpnet_cc_abi.h; the
 * element kinds of a volume are those of rpnet_prep_abi.h.  A library that carries these symbols says so: rpnet_smooth_abi_version() ==
 * RPNET_SMOOTH_ABI_VERSION.
 *
 * A volume is contiguous [D][H][W] float32 or int16, the RPNET_PREP_F32 / RPNET_PREP_I16 kinds; every axis length is 1..1024
 * (RPNET_CC_MAX_DIM).  fl(.) is one float64 rounding; csrc/smooth.hip is built with -ffp-contract=off, as resample.hip is built.
 *
 * Weights.  `wz`, `wy`, `wx` are 2r + 1 float64 weights each, in device memory, for the radii `rz`, `ry`, `rx` (0..RPNET_SMOOTH_MAX_RADIUS);
 * the host builds them (rpnet_amd.smooth.smooth_weights: scipy's kernel), so `exp` is the host's.  A table may be null exactly when its
 * radius is 0.
 * Passes.  The voxels are widened to float64.  The x pass runs first, then y, then z.  A pass with radius 0 is skipped; it is not a
 * multiplication by 1.  One pass along an axis of length `n`, for every line of the axis and every index `i` of the line:
 *     s = 0; for k = -r .. r ascending: s = fl(s + fl(w[k + r] * v[fold(i + k)]))
 *  - border = REFLECT: `j = (i + k) mod 2n` taken non-negative, then `fold = j >= n ? 2n - 1 - j : j`.  This is scipy's mode='reflect'
 *    (d c b a | a b c d | d c b a), of period 2n, for any radius, also one longer than the line.
 *  - border = NEAREST: `fold = clamp(i + k, 0, n - 1)`.  This is scipy's mode='nearest'.
 *  - Nothing is rounded to a narrower type between passes.  Where the intermediates live is the kernel's business.
 * Result.  One conversion to the kind of the volume at the end: float32 rounds to nearest; int16 rounds half to even and saturates to
 * [-32768, 32767].  With all three radii 0 the output is the input bit for bit.  A NaN or an infinity is not special-cased: it spreads
 * over its ball.
 * Anti-aliasing.  rpnet_amd.smooth.antialias_sigma gives an axis that shrinks from n to m voxels the sigma (n / m - 1) / 2 voxels, and an
 * axis that does not shrink none.  That rule is this project's own: scipy.ndimage.zoom has no prefilter for order 1, and the reference
 * ships none.
 * Not done.  No other kernel than the one the weights spell, no border modes beside the two, no volumes of more than one channel. */
#ifndef RPNET_SMOOTH_ABI_H
#define RPNET_SMOOTH_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"
#include "rpnet_cc_abi.h"
#include "rpnet_prep_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_SMOOTH_ABI_VERSION 1
int rpnet_smooth_abi_version(void);

/* border */
#define RPNET_SMOOTH_REFLECT 0 /* scipy mode='reflect': d c b a | a b c d | d c b a, period 2n, any radius */
#define RPNET_SMOOTH_NEAREST 1 /* scipy mode='nearest': index clamped to [0, n-1] */

#define RPNET_SMOOTH_MAX_RADIUS 255

/* The entry point launches on `stream` only: no allocation, no copy, no synchronisation, nothing read back, so a call can be captured in
 * a graph.  Every loop runs to a count fixed when it is entered; no block waits for another; there are no atomics, so two runs give the
 * same bits.
 *
 * The workspace is a 64-byte head (kept for the layout the other volume families have; nothing is stored in it) and B float64 volumes of
 * D * H * W values, each padded to 16 bytes, where P is the number of radii that are not 0 and B = min(2, max(0, P - 1)) the
 * intermediates between P passes (the second and the third pass cannot work in place):
 *     rpnet_smooth_workspace_bytes = 64 + 16 * ((D * H * W + 1) / 2) * B.
 * The query makes no GPU call and gives 0 and an error string for an extent below 1 or above RPNET_CC_MAX_DIM or a radius below 0 or
 * above RPNET_SMOOTH_MAX_RADIUS.  workspace: at least that many bytes, 16-byte aligned, used by one call at a time.
 *
 * The launches of a call: one per pass whose radius is not 0, x then y then z; the first reads `in`, the last writes `out`, the ones
 * between them write and read the float64 volumes of the workspace.  With all radii 0, one launch copies `in` to `out`.  A lane owns a
 * run of 16 bytes of consecutive x positions of the volume's kind (4 float32, 8 int16), read and written with 16-byte accesses where the
 * run is whole and its address 16-byte aligned (decided per lane) and element by element otherwise.
 *
 * rpnet_smooth_image   in, out: D*H*W elements of `kind`, aligned to the element; they must not overlap each other or the workspace.
 *   wz, wy, wx: 8-byte aligned.
 * Refused with a status and an error string, before anything is launched: a null pointer (a weight table may be null exactly when its
 * radius is 0), an unknown kind or border, an extent below 1 or above RPNET_CC_MAX_DIM, a radius below 0 or above RPNET_SMOOTH_MAX_RADIUS,
 * a workspace that is too small or not 16-byte aligned, a misaligned volume or weight table, an overlap. */
size_t rpnet_smooth_workspace_bytes(int D, int H, int W, int rz, int ry, int rx);
int rpnet_smooth_image(const void* in, int kind, int D, int H, int W, void* out, const double* wz, int rz, const double* wy, int ry,
                       const double* wx, int rx, int border, void* workspace, size_t workspace_bytes, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_SMOOTH_ABI_H */
