// HIP kernel (gfx950) of the BGZF reader; the per-member code is in inflate_core.h.
//
// Mapping: one wavefront per BGZF member, grid-strided over the members.  Lane 0 reads the bit stream (a serial thing) into a ring of 64
// tokens in LDS; the 64 lanes then write the ring's bytes, one byte of the output per lane and step.  The window of a member is its own
// slot of the output in HBM: a match reads what an earlier round of the same wave stored there, behind the fence, the wait and the barrier
// of INFL_SYNC.  6 KB of LDS (two lookup tables, the canonical arrays, a CRC table, the ring), so the waves of a CU are bounded by their
// slots, not by LDS: what hides lane 0's dependent loads is the number of members in flight.
#include "inflate_core.h"

static_assert(INFL_T == 64u, "a member's workgroup is one wavefront");

__global__ void __launch_bounds__(INFL_T) inflate_member_kernel(const infl_args_t G) {
    __shared__ infl_shared_t S;
    for (uint64_t b = blockIdx.x; b < G.n_members; b += gridDim.x) infl_member(S, G, b);
}
