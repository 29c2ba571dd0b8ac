// pp_wo_home.h -- the window a record starts in ("home"), the ONE rule the window-order mirror is built by and read by.
// Included by the reader (pp_k_direct.h: k_prepd finds where each window's entries start) and by the producer that works
// from a batch's arrays (pp_prepare.hip: pp_batch_prepare), so that the two cannot drift.  The other producers (pp_ingest.cpp
// window_of, pp_tokenize.hip k_tok_group) write the same rule out where they have the record in hand.
#pragma once

#include "pp_internal.h"

namespace pp {

// clamped: a record that starts beyond the assembly's last window belongs to the last one (c_lo = its contig's offset)
__device__ __forceinline__ uint32_t wo_home(unsigned long long c_lo, uint32_t ref_start, uint32_t nwin) {
    return (uint32_t)min((c_lo + ref_start) / (unsigned long long)TILE, (unsigned long long)(nwin - 1u));
}

}  // namespace pp
