// hk_arena_copy.hip -- the gfx950 copy kernel behind hk_snapshot / hk_restore / hk_copy_arenas (hk_arena_copy.h).
#include "hk_arena_copy.h"

namespace hk {

// One 64-lane workgroup copies 64 consecutive list entries.
//   rows       lane l owns entry l: its NFF + NPW + 3 scalar words (the SoA rows put the 64 lanes of a field on
//              consecutive words when the indices are consecutive)
//   manifolds  16-B quads, four lanes per 64-B record: in trip t lane l moves quad l & 3 of entry 16 t + (l >> 2),
//              so a destination list of consecutive arenas is written as whole contiguous segments (1 KiB per store
//              instruction) and a source arena repeated K times is read from HBM once and from L2 afterwards
// The validated indices travel from the rows' lane to the manifold lanes through LDS (-1: nothing to copy).
__global__ void __launch_bounds__(64) copy_arenas_kernel(ArenaView dst, const int64_t *dst_idx, ArenaView src,
                                                         const int64_t *src_idx, int64_t m, unsigned long long *bad) {
  __shared__ int64_t s_di[64], s_si[64];
  const int lane = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x * 64 + lane;
  int64_t di = -1, si = -1;
  bool rejected = false;
  if (e < m) {
    rejected = !copy_entry(dst, dst_idx, src, src_idx, e, di, si);
    if (rejected) di = si = -1;
  }
  const unsigned long long nb = __ballot(rejected);  // one atomic per wave that holds a bad entry
  if (nb && lane == __ffsll((long long)nb) - 1) atomicAdd(bad, (unsigned long long)__popcll(nb));
  if (di >= 0) copy_arena_rows(dst, di, src, si);
  s_di[lane] = di;
  s_si[lane] = si;
  __syncthreads();
  const int q = lane & (kRecQuads - 1);
#pragma unroll 1
  for (int t = 0; t < kRecQuads; ++t) {
    const int ent = t * (64 / kRecQuads) + lane / kRecQuads;
    const int64_t d = s_di[ent], s = s_si[ent];
    if (d >= 0) copy_arena_quads(dst, d, src, s, q);
  }
}

hipError_t launch_copy_arenas(const ArenaView &dst, const int64_t *dst_idx, const ArenaView &src,
                              const int64_t *src_idx, int64_t m, unsigned long long *bad, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(copy_arenas_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, dst, dst_idx, src, src_idx,
                     m, bad);
  return hipGetLastError();
}

}  // namespace hk
