// hk_seeded_reset.hip -- the gfx950 kernel behind hk_seeded_params / hk_reset_seeded: HockeyEnv.reset(seed=s)'s
// placement drawn on the device, one lane per arena (hk_seed.h: SeedSequence -> PCG64 -> placement_law).
#include "hk_kernels.h"

// the static scene (hk_kernels.hip's compile-time constant): the TRAIN_DEFENSE shot reads the puck's mass
constexpr hk::Scene g_scene =
#include "hk_scene_data.inc"
    ;

#include "hk_seed.h"

namespace hk {

// Lane a draws arena a's placement from seeds[a].  The puck side it draws for: one_in[a] when given; else the
// arena's stored one_starts flag (PW_TAW bit 31), toggled first when `toggle` (NORMAL mode only, as reset_lane
// toggles it).  Reads that one word of the arena and writes none.  Arenas outside the mask are skipped.
//   params [N,6], max_t [N] or NULL, one_out [N] or NULL (the side drawn for: reset_kernel's one_in)
__global__ void __launch_bounds__(64) seeded_params_kernel(DevState s, int mode, const uint8_t *mask,
                                                           const uint64_t *seeds, const uint8_t *one_in, int toggle,
                                                           float *params, int32_t *max_t, uint8_t *one_out) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= s.n) return;
  if (mask && !mask[a]) return;
  int one;
  if (one_in) {
    one = one_in[a] != 0;
  } else {
    one = (int)(reinterpret_cast<const uint32_t *>(s.i)[(int64_t)PW_TAW * s.n + a] >> 31);
    if (toggle && mode == 0) one = !one;
  }
  float p6[6];
  int mt;
  seeded_placement(seeds[a], mode, one, p6, mt);
#pragma unroll
  for (int k = 0; k < 6; ++k) params[a * 6 + k] = p6[k];
  if (max_t) max_t[a] = mt;
  if (one_out) one_out[a] = (uint8_t)one;
}

hipError_t launch_seeded_params(const DevState &s, const KCfg &cfg, const uint8_t *mask, const uint64_t *seeds,
                                const uint8_t *one_in, int toggle, float *params, int32_t *max_t, uint8_t *one_out,
                                hipStream_t st) {
  hipLaunchKernelGGL(seeded_params_kernel, dim3((unsigned)((s.n + 63) / 64)), dim3(64), 0, st, s, cfg.mode, mask, seeds,
                     one_in, toggle, params, max_t, one_out);
  return hipGetLastError();
}

}  // namespace hk
