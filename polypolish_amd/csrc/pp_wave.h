// pp_wave.h -- the wave-wide scan shared by the polish kernels (pp_kernels.hip, through pp_k_common.h) and the workgroup scans of
// pp_dev.h (the record chain: pp_bam.hip, pp_names.hip, pp_gate.hip), and the wave-wide 64-bit sum of the polish kernels and the
// text passes (pp_polish_text.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pp {

// Inclusive prefix sum over the wave's 64 lanes with data-parallel primitives (gfx9 DPP: shifts inside a row of 16 lanes, then
// lane 15 of a row to the next row, lane 31 to the upper half): six v_add with a DPP operand and no address registers, where
// six __shfl_up are six ds_bpermute with an index register each -- indices the compiler kept alive from k_tile's prologue to
// its prefix sums, in scratch memory across the item loop (round 6).
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2 and 3
    return v;
}

// The sum of a 64-bit value over the wave's 64 lanes, the same in every lane (a butterfly of shuffles).
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace pp
