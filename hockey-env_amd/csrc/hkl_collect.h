// hkl_collect.h -- collection on the device (the contract and the laws are in include/hockey_collect.h): hkl_opp_draw,
// player 2's opponent draw with one lane per arena, and hkl_collect, the replay store and the step's bookkeeping.
// Both grids are (workgroups of a member, member): a workgroup lies inside one member, so the member's words are
// workgroup-uniform and a row's rank among its member's running arenas is a prefix inside the member's workgroups.
#pragma once
#include "hkl_rng.h"

namespace hkl {

constexpr int CWG = 256;  // rows per workgroup of every kernel here

__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  return (double)((((uint64_t)a << 32) | b) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ void add64(int64_t *p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// ------------------------------------------------------------------------------------------------ opponent draw
__global__ void __launch_bounds__(CWG) opp_draw_kernel(hkl_opp_draw_io io) {
  __shared__ int32_t tot[3];
  const int n = io.rows_per_member, m = blockIdx.y, P = io.pmax;
  const int64_t local = (int64_t)blockIdx.x * CWG + threadIdx.x;
  if (threadIdx.x < 3) tot[threadIdx.x] = 0;
  __syncthreads();
  if (local < n) {
    const int64_t row = (int64_t)m * n + local;
    const uint64_t seed = io.seeds[m], calls = (uint64_t)io.calls[m];
    const P4 r = philox_at(seed ^ HKL_COLLECT_KEY_OPP, local, calls);
    int32_t L = io.len[m];
    L = L < 0 ? 0 : L > P ? P : L;
    const float *sc = io.scores + (int64_t)m * P;
    double total = 0.0;
    for (int k = 0; k < L; ++k) total += (double)sc[k];
    const bool can_sp = L > 0 && total > 0.0 && total < INFINITY;  // a NaN total fails both compares
    const bool sp = can_sp && u24(r.x) < io.probs[2 * m];
    const bool strong = !sp && u24(r.y) < io.probs[2 * m + 1];
    int32_t k = -1;
    if (sp) {
      const double t = dmul_rn(u53(r.z, r.w), total);
      double cum = 0.0;
      k = L - 1;
      for (int j = 0; j < L; ++j) {
        cum += (double)sc[j];
        if (cum > t) {
          k = j;
          break;
        }
      }
    }
    io.policy2[row] = sp ? HKL_P2_EXTERNAL : strong ? HKL_P2_STRONG : HKL_P2_WEAK;
    io.policy[row] = sp ? io.slots[(int64_t)m * P + k] : -1;
    io.snap[row] = sp ? m * P + k : -1;
    if (io.opp_inc) {
      const P4 q = philox_at(seed ^ HKL_COLLECT_KEY_PHASE, local, calls);
      io.opp_inc[2 * row] = 0.2 * u53(q.x, q.y);
      io.opp_inc[2 * row + 1] = 0.2 * u53(q.z, q.w);
    }
    if (!io.alive || io.alive[row]) {
      atomicAdd(&tot[sp ? 2 : strong ? 0 : 1], 1);
      if (sp) add64(io.snap_counts + (int64_t)m * P + k, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && tot[threadIdx.x]) add64(io.counts + 3 * m + threadIdx.x, tot[threadIdx.x]);
}

// one workgroup, lane m < S, after the draw in the stream: the only writer of calls
__global__ void __launch_bounds__(HKL_GROUP_MAX) opp_advance_kernel(hkl_opp_draw_io io, int n_members) {
  if ((int)threadIdx.x < n_members) io.calls[threadIdx.x] += 1;
}

// ------------------------------------------------------------------------------------------------ collect
// scratch: ticket[HKL_GROUP_MAX], then per (member, workgroup) bcnt[.][2] (alive rows, alive rows that go on), then
// bpre[.] (the member's alive rows in its earlier workgroups)
__host__ __device__ inline int collect_nb(int n) { return (n + CWG - 1) / CWG; }
struct CollectScratch {
  int32_t *ticket, *bcnt, *bpre;
};
__device__ __forceinline__ CollectScratch collect_scratch(const hkl_collect_io &io) {
  const int64_t sb = (int64_t)(io.n_rows / io.rows_per_member) * collect_nb(io.rows_per_member);
  return CollectScratch{io.scratch, io.scratch + HKL_GROUP_MAX, io.scratch + HKL_GROUP_MAX + 2 * sb};
}

// the member's state after a push of cnt rows, of which `after` go on: one thread
__device__ __forceinline__ void collect_commit(const hkl_collect_io &io, int m, int32_t cnt, int32_t after) {
  const int64_t pos = io.pos[m];
  const bool ok = pos >= 0 && pos < io.cap;
  io.push_pos[m] = ok ? pos : 0;
  io.push_n[m] = ok ? cnt : 0;
  if (ok) {
    const int64_t sz = io.size[m] < 0 ? 0 : io.size[m];
    io.pos[m] = (pos + cnt) % io.cap;
    io.size[m] = sz + cnt < io.cap ? sz + cnt : io.cap;
  }
  io.steps[m] += cnt;
  if (io.live && cnt > 0) io.live[m] += 1;
  if (io.alive) io.count[m] = after;
}

__global__ void __launch_bounds__(CWG) collect_count_kernel(hkl_collect_io io) {
  __shared__ int32_t c[2];
  const int n = io.rows_per_member, m = blockIdx.y;
  const int64_t local = (int64_t)blockIdx.x * CWG + threadIdx.x;
  if (threadIdx.x < 2) c[threadIdx.x] = 0;
  __syncthreads();
  if (local < n) {
    const int64_t row = (int64_t)m * n + local;
    if (io.alive[row]) {
      atomicAdd(&c[0], 1);
      if (!io.done[row]) atomicAdd(&c[1], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) collect_scratch(io).bcnt[2 * ((int64_t)m * gridDim.x + blockIdx.x) + threadIdx.x] = c[threadIdx.x];
}

// exclusive prefix of v over the workgroup's CWG threads (s: CWG ints); returns the prefix, total receives the sum
__device__ __forceinline__ int32_t block_exclusive(int32_t v, int32_t *s, int32_t &total) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < CWG; d <<= 1) {
    const int32_t add = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const int32_t incl = s[t];
  total = s[CWG - 1];
  __syncthreads();
  return incl - v;
}

// one workgroup per member: the prefix of its workgroups' alive counts, then the member's commit
__global__ void __launch_bounds__(CWG) collect_scan_kernel(hkl_collect_io io) {
  __shared__ int32_t s[CWG];
  const int m = blockIdx.x, nb = collect_nb(io.rows_per_member);
  const CollectScratch sc = collect_scratch(io);
  int32_t carry = 0, after = 0;
  for (int base = 0; base < nb; base += CWG) {
    const int b = base + threadIdx.x;
    const int64_t at = (int64_t)m * nb + b;
    const int32_t v = b < nb ? sc.bcnt[2 * at] : 0, go = b < nb ? sc.bcnt[2 * at + 1] : 0;
    int32_t total, total_go;
    const int32_t pre = block_exclusive(v, s, total);
    block_exclusive(go, s, total_go);
    if (b < nb) sc.bpre[at] = carry + pre;
    carry += total;
    after += total_go;
  }
  if (threadIdx.x == 0) collect_commit(io, m, carry, after);
}

// Ranked: alive given, after collect_count_kernel and collect_scan_kernel (pos is already the next push's: the push's
// own start is push_pos).  Else every row is alive, rank = local, and the member's last workgroup commits.
template <bool Ranked>
__global__ void __launch_bounds__(CWG) collect_store_kernel(hkl_collect_io io) {
  __shared__ int32_t s[CWG];
  __shared__ int64_t dsts[CWG];
  __shared__ bool last;
  const int n = io.rows_per_member, m = blockIdx.y, t = threadIdx.x;
  const int64_t local = (int64_t)blockIdx.x * CWG + t;
  const int64_t row0 = (int64_t)m * n + (int64_t)blockIdx.x * CWG;  // the workgroup's first row
  const int rows = n - (int64_t)blockIdx.x * CWG < CWG ? (int)(n - (int64_t)blockIdx.x * CWG) : CWG;
  const int64_t row = row0 + t;
  const bool valid = local < n;
  const CollectScratch sc = collect_scratch(io);
  const int64_t pos = Ranked ? io.push_pos[m] : io.pos[m];
  const bool ok = pos >= 0 && pos < io.cap && (!Ranked || io.push_n[m] > 0);
  const bool alive = valid && (!Ranked || io.alive[row]);
  int64_t rank = local;
  if (Ranked) {
    int32_t total;
    rank = (int64_t)sc.bpre[(int64_t)m * gridDim.x + blockIdx.x] + block_exclusive(alive ? 1 : 0, s, total);
  }
  int64_t dst = -1;
  if (alive && ok && rank >= 0 && rank < n) dst = (int64_t)m * io.cap + (pos + rank) % io.cap;  // n <= cap
  dsts[t] = dst;
  if (valid) {
    const float rw = io.reward[row];
    const bool dn = io.done[row] != 0;
    if (dst >= 0) {
      io.r[dst] = rw;
      io.d[dst] = dn ? 1.0f : 0.0f;
#pragma unroll
      for (int c = 0; c < 4; ++c) io.a[dst * 4 + c] = io.act[row * io.act_ld + c];
    }
    io.ep_reward[row] = fadd_rn(io.ep_reward[row], alive ? rw : 0.0f);
    if (alive && dn && io.snap) {
      const int32_t sn = io.snap[row];
      if (sn >= 0 && sn < (io.n_rows / n) * io.pmax) add64(io.tally + 2 * (int64_t)sn + (rw > 0.0f ? 0 : 1), 1);
    }
    if (Ranked && dn) io.alive[row] = 0;
  }
  __syncthreads();
  // the observation rows, float by float: thread t reads float e of obs and obs_next, and only then stores keep_obs's
  for (int e = t; e < rows * 18; e += CWG) {
    const int64_t at = row0 * 18 + e, d18 = dsts[e / 18] * 18 + e % 18;
    const float o = io.obs[at], o2 = io.obs_next[at];
    if (d18 >= 0) {
      io.s[d18] = o;
      io.s2[d18] = o2;
    }
    if (io.keep_obs) io.keep_obs[at] = o2;
    if (io.keep_obs2) io.keep_obs2[at] = io.obs2_next[at];
  }
  if (!Ranked) {
    // every workgroup has read pos by now; the fence orders that read before the ticket, and the last one commits
    __syncthreads();
    if (t == 0) {
      __threadfence();
      last = atomicAdd(&sc.ticket[m], 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (last && t == 0) {
      sc.ticket[m] = 0;
      collect_commit(io, m, n, n);
    }
  }
}

}  // namespace hkl
