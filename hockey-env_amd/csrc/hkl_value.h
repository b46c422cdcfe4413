// hkl_value.h -- the twin-critic inference kernel of the learner library (hk_learner.hip).
// hkl_value: min(Q1, Q2) of a TD3 agent outside the learner, one launch.  act_kernel's geometry without the grouping:
// 256 threads and 64 rows per workgroup, one sample per 4 lanes; a partly filled last workgroup recomputes its last
// row in the spare lanes and stores nothing for them.  Q mode reads the row's action; V mode runs the actor forward
// first exactly as act_kernel does (gemm_in / gemm256 / gemm_out, a = tanh_fast(pre)) and keeps the action in
// registers -- critic_step_kernel's target path with zero noise, where the clamp is the identity (|tanh| <= 1).  Then
// both critics run through q_forward on the same first-layer fragments, one network's operands in LDS at a time.
//
// A row's results do not depend on the other rows or on its position, for act_kernel's reason: in a 16x16x4 MFMA a
// sample's output column is a function of its own B column alone, and every sample's k-steps run in the same order;
// head1 and gemm_out's broadcast only add and move values among the 4 lanes of one sample, in a fixed order.  The
// action enters unscale() and input_frags() through the same instructions in both modes, so Q mode on V mode's
// act_out gives V mode's q1 / q2 bit for bit.
//
// Two workgroups per CU (launch bound 2): head1's 32 float4 loads of w3 and the bias on top of the layer routines' 228
// registers ask for 272, and at that size one wave per SIMD waits alone at every barrier of gemm256.  Held to 256 the
// compiler spills 31 VGPRs (100 B of scratch per lane), and the second resident workgroup more than pays for them:
// 0.297 against 0.340 ms in V mode and 0.182 against 0.216 ms in Q mode at 65 536 rows.
#pragma once
#include "hkl_td3.h"

namespace hkl {

__global__ void __launch_bounds__(WG, 2) value_kernel(hkl_value_io io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];  // two fragment buffers + the staged bias
  const int64_t start = 64 * (int64_t)blockIdx.x;
  const int64_t cnt = io.n_rows - start;  // >= 1: the grid is ceil(n_rows / 64)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const int r = wave * 16 + j;
  const bool live = r < cnt;
  const int64_t row = start + (live ? r : cnt - 1);
  const float *orow = io.obs + row * io.obs_ld;
  float x[S1];
  Tile h1, h2;
  f4 a;
  if (io.act) {  // uniform over the grid
    const float *arow = io.act + row * io.act_ld;
    a = f4{arow[0], arow[1], arow[2], arow[3]};
  } else {
    const Net an = net_of(io.actor);
    input_frags(orow, z4(), false, x, q);
    gemm_in(an.f1(), x, h1, lane, sfrag);
    gemm256(an.fp(), h1, an.b1, h2, lane, sfrag);
    const f4 pre = gemm_out(an.fo(), h2, an.b2, an.b3, 4, lane, sfrag);
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = tanh_fast(pre[c]);
    // the sample's 4 lanes hold the same action: lane q stores component q
    if (io.act_out && live) io.act_out[row * io.act_out_ld + q] = q == 0 ? a[0] : q == 1 ? a[1] : q == 2 ? a[2] : a[3];
  }
  f4 au;
#pragma unroll
  for (int c = 0; c < 4; ++c) au[c] = unscale(a[c], io.act_low[c], io.act_range[c]);
  input_frags(orow, au, true, x, q);
  const float q0 = q_forward(net_of(io.q[0]), x, h1, h2, lane, sfrag);
  const float q1 = q_forward(net_of(io.q[1]), x, h1, h2, lane, sfrag);
  if (live && q == 0) {  // the sample's 4 lanes agree bit for bit (head1): one of them stores
    if (io.q1) io.q1[row] = q0;
    if (io.q2) io.q2[row] = q1;
    if (io.qmin) io.qmin[row] = fminf(q0, q1);
  }
}

}  // namespace hkl
