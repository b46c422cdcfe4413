// hkl_explore.h -- hkl_explore: hkl_act with TD3.act's exploration as the acting tile's epilogue (the contract and the
// law are in include/hockey_learner.h).  explore_kernel is act_kernel with ExploreEpi in place of the store: the
// grouping launches, the tile and with them a row's four actor outputs are hkl_act's.  The epilogue reads the member's
// parameters and counters (wave-divergent only where a tile spans members) and writes the row's own floats: out, the OU
// state and z_out.  explore_advance_kernel, one workgroup after it in the stream, is the only writer of total / calls.
#pragma once
#include "hkl_act.h"
#include "hkl_rng.h"

namespace hkl {

// what the member's counters say about this call: the law's T0, T1 and all_random
struct ExplorePhase {
  int64_t t0, t1;
  bool all_random;
};
__device__ __forceinline__ ExplorePhase explore_phase(const hkl_explore_io &io, const hkl_explore_member &mem, int m) {
  const int64_t t = io.total[m];
  const int32_t c = io.count[m];
  ExplorePhase p;
  p.t0 = t < 0 ? 0 : t;
  p.t1 = p.t0 + (c < 0 ? 0 : c > io.rows_per_member ? io.rows_per_member : c);
  p.all_random = p.t1 < mem.start_steps;
  return p;
}
// TD3.noise_scale() at total_steps = t1, in float64, rounded once
__device__ __forceinline__ float explore_scale(const hkl_explore_member &mem, int64_t t1) {
  double s = mem.init_scale;
  if (mem.anneal != HKL_ANNEAL_NONE && mem.max_total_steps > 0) {
    const double r = (double)t1 / (double)mem.max_total_steps, progress = r < 1.0 ? r : 1.0;
    s = mem.anneal == HKL_ANNEAL_LINEAR ? mem.init_scale * (1.0 - progress) : mem.init_scale * pow(0.1, progress);
    s = s > mem.min_scale ? s : mem.min_scale;
  }
  return (float)s;
}

struct ExploreEpi {
  const hkl_explore_io &io;
  __device__ __forceinline__ void operator()(const hkl_act_io &act, int64_t row, int q, bool live, float a) const {
    const int n = io.rows_per_member;
    const int m = (int)(row / n);  // row < n_rows = S n
    const int64_t local = row - (int64_t)m * n;
    const hkl_explore_member mem = io.members[m];
    const ExplorePhase ph = explore_phase(io, mem, m);
    const uint64_t calls = (uint64_t)io.calls[m];
    float res = 0.0f, raw = 0.0f;
    if (!ph.all_random) {
      float unit = 0.0f;
      if (mem.noise == HKL_NOISE_GAUSSIAN || mem.noise == HKL_NOISE_OU || mem.noise == HKL_NOISE_UNIFORM) {
        const P4 r = philox_at(mem.seed ^ HKL_EXPLORE_KEY_NOISE, local, calls);
        if (mem.noise == HKL_NOISE_UNIFORM) {
          const uint32_t w = q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
          raw = 2.0f * u24(w) - 1.0f;
          unit = fmul_rn(raw, 1.7320508075688772f);
        } else {
          float z[4];
          box_muller(r, z);
          raw = q == 0 ? z[0] : q == 1 ? z[1] : q == 2 ? z[2] : z[3];
          unit = raw;
          if (mem.noise == HKL_NOISE_OU) {
            const float x = io.x[row * 4 + q];
            unit = fadd_rn(fadd_rn(x, fmul_rn(fmul_rn(mem.theta, -x), mem.dt)), fmul_rn(mem.sqrt_dt, raw));
            if (live) io.x[row * 4 + q] = unit;
          }
        }
      } else if (mem.noise == HKL_NOISE_EXTERNAL) {
        unit = io.ext[row * io.ext_ld + q * io.ext_cs];
      }
      const float v = fadd_rn(a, fmul_rn(unit, explore_scale(mem, ph.t1)));
      res = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;  // NaN compares false twice and stays
    }
    if (ph.all_random || ph.t0 + 1 + local < mem.start_steps) {
      const P4 r = philox_at(mem.seed ^ HKL_EXPLORE_KEY_RANDOM, local, calls);
      const uint32_t w = q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
      res = 2.0f * u24(w) - 1.0f;
    }
    if (live) {
      act.out[row * act.out_ld + act.out_col + q] = res;
      if (io.z_out) io.z_out[row * 4 + q] = raw;
    }
  }
};

// counts[0 .. HKL_ACT_MAX_POLICIES] := 0 before the histogram.  A kernel where hkl_act has a memset: replayed from a
// captured graph a memset node left the counters unzeroed ("Grouping for a large K"), the cursors of the
// last call then stood in for zeros, the scan's offsets ran past n_rows and the scatter and the acting tile addressed
// `order` out of bounds.  As a kernel node the step replays like the others, and the call is a line of kernel nodes.
__global__ void __launch_bounds__(128) explore_zero_kernel(hkl_act_io io) {
  if (threadIdx.x <= HKL_ACT_MAX_POLICIES) io.counts[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(WG, 1) explore_kernel(hkl_explore_io io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];
  int k, start, cnt;
  if (!act_locate(io.act, k, start, cnt)) return;
  // what the grouping left in its scratch is range-checked before it addresses anything (uniform over the workgroup)
  if (start < 0 || cnt <= 0 || start > io.act.n_rows - (cnt < 64 ? cnt : 64)) return;
  act_tile(io.act, k, start, cnt, sfrag, ExploreEpi{io});
}

// one workgroup, lane m < S: the member's counters after the call, and its scale
__global__ void __launch_bounds__(HKL_GROUP_MAX) explore_advance_kernel(hkl_explore_io io, int n_members) {
  const int m = threadIdx.x;
  if (m >= n_members) return;
  const hkl_explore_member mem = io.members[m];
  const ExplorePhase ph = explore_phase(io, mem, m);
  if (io.scale_out) io.scale_out[m] = explore_scale(mem, ph.t1);
  io.total[m] = ph.t1;
  io.calls[m] += 1;
}

}  // namespace hkl
