// The one reader of a volume element of the four accepted kinds (RPNET_SURFACE_U8 / I32 / I64 / F32 of include/rpnet_surface_abi.h; the
// RPNET_CC_* names of include/rpnet_cc_abi.h carry the same values, which cc_phases.h asserts): surface.hip, surface_spacing.hip,
// components.hip and cc_post.hip all read their volumes through it.
#ifndef RPNET_VOLUME_KINDS_H
#define RPNET_VOLUME_KINDS_H

#include "common.h"
#include "rpnet_surface_abi.h"

namespace rpnet {

// value == cls
__device__ __forceinline__ bool vol_fg(const void* p, const int kind, const size_t i, const int cls) {
    switch (kind) {
        case RPNET_SURFACE_U8: return (int)static_cast<const uint8_t*>(p)[i] == cls;
        case RPNET_SURFACE_I32: return static_cast<const int32_t*>(p)[i] == cls;
        case RPNET_SURFACE_I64: return static_cast<const int64_t*>(p)[i] == (int64_t)cls;
        default: return static_cast<const float*>(p)[i] == (float)cls;
    }
}
// the value as the uint8 a filtered volume is written in
__device__ __forceinline__ uint8_t vol_u8(const void* p, const int kind, const size_t i) {
    switch (kind) {
        case RPNET_SURFACE_U8: return static_cast<const uint8_t*>(p)[i];
        case RPNET_SURFACE_I32: return (uint8_t)static_cast<const int32_t*>(p)[i];
        case RPNET_SURFACE_I64: return (uint8_t)static_cast<const int64_t*>(p)[i];
        default: return (uint8_t)(int)static_cast<const float*>(p)[i];
    }
}

}  // namespace rpnet
#endif  // RPNET_VOLUME_KINDS_H
