// hkl_eval.h -- evaluation on the device (the contract and the laws are in include/hockey_eval.h): hkl_eval_begin and
// hkl_eval_step, the accounting of the evaluation loop with one lane per arena row, and hkl_eval_fold, one workgroup
// per cell.  The row grids are (workgroups of a cell, cell): a workgroup lies inside one cell, so the cell's seed is
// workgroup-uniform and a wave's finished rows belong to one count.
#pragma once
#include "hkl_collect.h"  // CWG, u53, philox_at

namespace hkl {

// opp_inc[row] = inc(c, local, t): the cell's phase increments of step t
__device__ __forceinline__ void eval_inc(const hkl_eval_io &io, int64_t row, uint64_t seed, int64_t local, uint64_t t) {
  const P4 q = philox_at(seed ^ HKL_EVAL_KEY_PHASE, local, t);
  io.opp_inc[2 * row] = 0.2 * u53(q.x, q.y);
  io.opp_inc[2 * row + 1] = 0.2 * u53(q.z, q.w);
}

__global__ void __launch_bounds__(CWG) eval_begin_kernel(hkl_eval_io io) {
  const int n = io.rows_per_cell, c = blockIdx.y;
  const int64_t local = (int64_t)blockIdx.x * CWG + threadIdx.x;
  if (local < n) {
    const int64_t row = (int64_t)c * n + local;
    io.live[row] = 1;
    io.ret[row] = 0.0;
    io.length[row] = 0;
    io.winner[row] = 0;
    if (io.opp_inc) eval_inc(io, row, io.seeds[c], local, 0);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    io.count[c] = n;
    if (c == 0) io.step[0] = 0;
  }
}

__global__ void __launch_bounds__(CWG) eval_step_kernel(hkl_eval_io io) {
  const int n = io.rows_per_cell, c = blockIdx.y;
  const int64_t local = (int64_t)blockIdx.x * CWG + threadIdx.x;
  const uint64_t t = (uint64_t)io.step[0];
  bool finished = false;
  if (local < n) {
    const int64_t row = (int64_t)c * n + local;
    if (io.live[row]) {
      io.ret[row] += (double)io.reward[row];
      io.length[row] += 1;
      if (io.done[row]) {
        const float f = io.info[row * io.info_ld];
        io.winner[row] = f > 0.0f ? 1 : f < 0.0f ? -1 : 0;
        io.live[row] = 0;
        finished = true;
      }
    }
    if (io.opp_inc) eval_inc(io, row, io.seeds[c], local, t + 1);
  }
  // every lane of the wave arrives here: the wave's finished rows leave the cell's count in one atomic
  const int gone = __popcll(__ballot(finished));
  if ((threadIdx.x & 63) == 0 && gone) atomicSub(&io.count[c], gone);
}

// one thread, after the step kernel in the stream: the only writer of step
__global__ void eval_advance_kernel(hkl_eval_io io) { io.step[0] += 1; }

// one workgroup per cell
__global__ void __launch_bounds__(CWG) eval_fold_kernel(hkl_eval_io io) {
  __shared__ double p[CWG];
  __shared__ int64_t q[5][CWG];  // winner +1, 0, -1, live rows, length sum
  const int n = io.rows_per_cell, c = blockIdx.x, l = threadIdx.x;
  double sum = 0.0;
  int64_t k[5] = {0, 0, 0, 0, 0};
  for (int64_t j = l; j < n; j += CWG) {
    const int64_t row = (int64_t)c * n + j;
    if (io.live[row]) {
      k[3] += 1;
    } else {
      const int w = io.winner[row];
      sum += io.ret[row];
      k[0] += w > 0;  // constant indices: k stays in registers
      k[1] += w == 0;
      k[2] += w < 0;
      k[4] += io.length[row];
    }
  }
  p[l] = sum;
#pragma unroll
  for (int a = 0; a < 5; ++a) q[a][l] = k[a];
  __syncthreads();
  for (int s = CWG / 2; s >= 1; s >>= 1) {
    if (l < s) {
      p[l] += p[l + s];
#pragma unroll
      for (int a = 0; a < 5; ++a) q[a][l] += q[a][l + s];
    }
    __syncthreads();
  }
  if (l < 4) io.outcomes[4 * (int64_t)c + l] = q[l][0];
  if (l == 4) io.length_sum[c] = q[4][0];
  if (l == 5) io.return_sum[c] = p[0];
}

}  // namespace hkl
