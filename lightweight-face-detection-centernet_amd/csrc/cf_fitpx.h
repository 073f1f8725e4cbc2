// The pieces of the fit kernel (cf_fit.hip) that the rotated fit (cf_rot.hip) shares: the byte-selecting pack of one pixel and the
// three-dword store of four canvas pixels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cf {

// Three values 0..255 -> B | G << 8 | R << 16 by byte selection from whole dwords (two v_perm_b32).  Written as shifts and ORs, the
// clamp of cv_linear_vpass next to the packing is selected as gfx950's v_ashr_pk_u8_i32, whose result came back from the device with
// foreign bits above bit 15 in this kernel (they reach R and the next pixel's B); a byte selection takes bits 7:0 of each value and
// nothing else.
__device__ __forceinline__ uint32_t pack_bgr(uint32_t b, uint32_t g, uint32_t r) {
    const uint32_t bg = __builtin_amdgcn_perm(g, b, 0x0c0c0400u);       // byte 0 = b[7:0], byte 1 = g[7:0], bytes 2, 3 = 0
    return __builtin_amdgcn_perm(r, bg, 0x0c040100u);                   // bytes 0, 1 = bg[15:0], byte 2 = r[7:0], byte 3 = 0
}

__device__ __forceinline__ void fit_store(uint8_t* row, const uint32_t (&p)[4]) {
    uint32_t* o = reinterpret_cast<uint32_t*>(row);
    o[0] = p[0] | (p[1] << 24);
    o[1] = (p[1] >> 8) | (p[2] << 16);
    o[2] = (p[2] >> 16) | (p[3] << 8);
}

}  // namespace cf
