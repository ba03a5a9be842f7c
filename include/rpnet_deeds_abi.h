/* C ABI of the DEEDS registration entry points of librpnet_hip.so: the third registration stage of the reference (net/registration.py
 * DEEDSRegistration, :360-381 and :412-471) for all slices of a volume at once (csrc/deeds.hip; rpnet_amd/registration.py).  One pass,
 * no optimiser: a cost per grid point and displacement, regularised, and a softmax expectation of the displacements; a second
 * element-wise launch warps an image by the resulting sampling grid.
 *
 * A header of its own beside rpnet_abi.h and the twelve side headers before it, none of which it changes; its ledger of tests is
 * tests/deeds_abi_ledger.py, held to the rules of tests/abi_ledger.py by tests/test_host_deeds_abi_ledger.py.  Status codes,
 * rpnet_stream_t and rpnet_last_error_string() are those of rpnet_abi.h.  A library that carries these symbols says so:
 * rpnet_deeds_abi_version() == RPNET_DEEDS_ABI_VERSION.
 *
 * Definition (PyTorch defaults: align_corners=False, zero padding; R = disp_range, a0..a5 = alpha; all float32).
 *   grid points    p = (gi, gj), 0 <= gi, gj < G, at (x, y) = (gbase[gj], gbase[gi])
 *   displacements  d = di * D + dj, 0 <= di, dj < D, of (x, y) = (R * sbase[dj], R * sbase[di])
 *   dc[p][d]       = a1 + a0 * (fixed(p) - moving(p + d))^2, both sampled bilinearly, a corner outside the image reads as zero
 *   minconv(c)     per p over the (di, dj) plane: replicate pad 3, 3x3 minimum, 3x3 average, 3x3 average
 *   meanfield(c)   per d over the (gi, gj) plane: replicate pad 2, 3x3 average, 3x3 average (evaluated as one 5x5 filter with the taps
 *                  (1 2 3 2 1) x (1 2 3 2 1) / 81 over indices clamped to the grid)
 *   cost           = meanfield(minconv(a4 + a2 * dc + a3 * meanfield(minconv(dc))))         [S][G*G][D*D], what cost_out receives
 *   pred[p]        = sum_d softmax_d(-a5 * cost[p][d]) * displacement(d)                    [S][G][G][2], (x, y)
 * gbase [G] and sbase [D] are the 1-D base grids of F.affine_grid (torch.linspace(-1, 1, n) * (n - 1) / n), taken by the host from
 * torch so that sample positions round as the reference's do.
 *
 * Warp.  The sampling grid (gbase + pred) [G][G][2] is brought to H x W by torch's legacy `nearest` rule
 * (source index = min(floor(i * (float)G / H), G - 1)) or by `bilinear` with align_corners=False
 * (source position = max((float)G / H * (i + 0.5) - 0.5, 0)); out = [threshold](scale * sample(x) + shift), threshold < 0 for none,
 * as rpnet_affine_warp. */
#ifndef RPNET_DEEDS_ABI_H
#define RPNET_DEEDS_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rpnet_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPNET_DEEDS_ABI_VERSION 1
int rpnet_deeds_abi_version(void);

#define RPNET_DEEDS_MAX_GRID 512  /* 1 <= G <= 512 */
#define RPNET_DEEDS_MAX_WIDTH 31  /* D odd, 1 <= D <= 31 */

/* how rpnet_deeds_warp brings the sampling grid to the image's extent */
#define RPNET_DEEDS_NEAREST 0
#define RPNET_DEEDS_BILINEAR 1

/* The entry points launch on `stream` only: no allocation, no copy, no synchronisation, nothing read back, so every call can be captured
 * in a graph.  No atomics; every loop runs to a count fixed when it is entered; no block waits for another; two runs give the same bits.
 *
 * Launches.  register with a3 == 0: one per 32768 slices; the cost volume stays in LDS.  register with a3 != 0 (`general`): two per
 * chunk of slices, the first path's mean field goes through the workspace:
 *     rpnet_deeds_workspace_bytes = general ? min(S, max(1, min(32768, 2^28 / (G*G*D*D*4)))) * G*G*D*D*4 : 0
 * The query makes no GPU call and gives 0 and an error string for S < 0 or G, D outside their limits.  warp: one per 32768 slices.
 *
 * rpnet_deeds_register  moving, fixed: S*H*W float32.  gbase: G, sbase: D float32.  pred: S*G*G*2 float32.  cost_out: null or
 *   S*G*G*D*D float32.  ws: at least rpnet_deeds_workspace_bytes(S, G, D, a3 != 0) bytes, 4-byte aligned, used by one call at a
 *   time; may be null where that is 0.
 * rpnet_deeds_warp      x, out: S*H*W float32, disjoint.  pred: S*G*G*2 float32.  gbase: G float32.  mode: RPNET_DEEDS_NEAREST or
 *   RPNET_DEEDS_BILINEAR.
 * Refused with a status and an error string, before anything is launched: a null pointer, S < 0, H or W below 2, H*W >= 2^30, G
 * outside 1..512, D even or outside 1..31, a disp_range or alpha that is not finite, a workspace that is too short, an unknown mode.
 * S == 0 returns RPNET_OK and launches nothing. */
size_t rpnet_deeds_workspace_bytes(int S, int G, int D, int general);
int rpnet_deeds_register(const float* moving, const float* fixed, const float* gbase, const float* sbase, int S, int H, int W, int G, int D,
                         float disp_range, float alpha0, float alpha1, float alpha2, float alpha3, float alpha4, float alpha5, float* pred,
                         float* cost_out, void* ws, size_t ws_bytes, rpnet_stream_t stream);
int rpnet_deeds_warp(const float* x, const float* pred, const float* gbase, float* out, int S, int H, int W, int G, int mode, float threshold,
                     float scale, float shift, rpnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RPNET_DEEDS_ABI_H */
