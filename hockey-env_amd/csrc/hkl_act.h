// hkl_act.h -- the acting kernels of the learner library (hk_learner.hip): hkl_act and hkl_act_wide.
// hkl_act: the actor forward tanh(W3 tanh(W2 tanh(W1 obs + b1) + b2) + b3) of actor_step_kernel's first third, for
// acting: every row of a batch runs the policy its `policy` entry names out of a bank of K (self-play pools,
// cross-play).  The layer routines stage ONE network's fragments in LDS for the 4 waves of a workgroup, so the rows
// are first grouped by policy on the device and every workgroup takes 64 rows of one group:
//   act_hist_kernel     counts[k] = rows of policy k: a histogram per workgroup in LDS, then one global atomic per
//                       (workgroup, occupied k);
//   act_scan_kernel     offsets = the exclusive scan of the K counts (offsets[K] = the rows that act), counts := 0;
//   act_scatter_kernel  order[offsets[k] + ..] = the rows of policy k: a workgroup reserves its rows' range with one
//                       atomic per occupied k on counts (now the groups' cursors) and ranks them in LDS;
//   act_kernel          workgroup b walks the offsets to its (policy, 64-row chunk) and runs gemm_in / gemm256 /
//                       gemm_out on the gathered rows.
// The order of the rows inside a group depends on the atomics' timing; the results do not: in a 16x16x4 MFMA a
// sample's output column is a function of its own B column alone, and every sample's k-steps run in the same order,
// so a row's four outputs are the same bits wherever it sits and whoever its tile-mates are.
#pragma once
#include "hkl_mlp.h"

namespace hkl {

constexpr int kActW1 = 0, kActB1 = kActW1 + H * 18, kActW2 = kActB1 + H, kActB2 = kActW2 + H * H, kActW3 = kActB2 + H,
              kActB3 = kActW3 + 4 * H;
static_assert(kActB3 + 4 == HKL_ACT_PARAM_FLOATS, "parameter block (include/hockey_learner.h)");
static_assert(HKL_ACT_PARAM_FLOATS % 4 == 0 && HKL_PACK_FLOATS % 4 == 0, "bank slots keep 16-byte alignment");

// a row's policy, or -1 for a row that does not act (any id outside [0, K) is treated as -1: no lane indexes the
// tables with it)
__device__ __forceinline__ int act_policy(const hkl_act_io &io, int i) {
  const int k = io.policy[i];
  return (k >= 0 && k < io.n_policies) ? k : -1;
}

__global__ void __launch_bounds__(256) act_hist_kernel(hkl_act_io io) {
  __shared__ int h[HKL_ACT_MAX_POLICIES];
  if (threadIdx.x < HKL_ACT_MAX_POLICIES) h[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int k = i < io.n_rows ? act_policy(io, i) : -1;
  if (k >= 0) atomicAdd(&h[k], 1);
  __syncthreads();
  if (threadIdx.x < io.n_policies && h[threadIdx.x]) atomicAdd(&io.counts[threadIdx.x], h[threadIdx.x]);
}

// one wave: a Kogge-Stone scan over the (at most 64) counts
__global__ void __launch_bounds__(64) act_scan_kernel(hkl_act_io io) {
  const int l = threadIdx.x;
  const int c = l < io.n_policies ? io.counts[l] : 0;
  int s = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(s, d);
    if (l >= d) s += t;
  }
  if (l < io.n_policies) {
    io.offsets[l] = s - c;
    io.counts[l] = 0;  // the scatter's cursors
  }
  if (l == io.n_policies - 1) io.offsets[io.n_policies] = s;
}

__global__ void __launch_bounds__(256) act_scatter_kernel(hkl_act_io io) {
  __shared__ int h[HKL_ACT_MAX_POLICIES], base[HKL_ACT_MAX_POLICIES];
  if (threadIdx.x < HKL_ACT_MAX_POLICIES) h[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int k = i < io.n_rows ? act_policy(io, i) : -1;
  const int rank = k >= 0 ? atomicAdd(&h[k], 1) : 0;
  __syncthreads();
  if (threadIdx.x < io.n_policies && h[threadIdx.x])
    base[threadIdx.x] = io.offsets[threadIdx.x] + atomicAdd(&io.counts[threadIdx.x], h[threadIdx.x]);
  __syncthreads();
  if (k >= 0) io.order[base[k] + rank] = i;  // < offsets[k + 1] <= n_rows: the hist pass counted the same rows
}

// One acting tile: policy k on the rows order[start .. start + min(cnt, 64)) (policy == NULL: the rows themselves).
// IO is hkl_act_io or hkl_act_wide_io; act_kernel and act_wide_kernel differ only in how a workgroup finds (k, start,
// cnt), so a row's four outputs are the same bits under either.  k, start and cnt are uniform over the workgroup.
// Epi is what happens to the action a lane is about to store: epi(io, row, q, live, a), called by every lane (a spare
// lane, live == false, must store nothing).  ActStore, the default, is the store itself; hkl_explore.h passes the
// exploration epilogue.
struct ActStore {
  template <class IO>
  __device__ __forceinline__ void operator()(const IO &io, int64_t row, int q, bool live, float a) const {
    if (live) io.out[row * io.out_ld + io.out_col + q] = a;
  }
};
template <class IO, class Epi = ActStore>
__device__ __forceinline__ void act_tile(const IO &io, int k, int start, int cnt, f4 *sfrag, const Epi &epi = Epi()) {
  if (cnt <= 0) return;  // (never taken: a tile holds at least one row)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  // a partly filled workgroup: its spare lanes recompute the group's last row of this chunk and store nothing
  const int r = wave * 16 + j;
  const bool live = r < cnt;
  const int pos = start + (live ? r : cnt - 1);
  const int64_t row = io.policy ? io.order[pos] : pos;
  const float *par = io.params + (int64_t)k * HKL_ACT_PARAM_FLOATS;
  const Net an{par + kActW1, par + kActB1, par + kActW2, par + kActB2, par + kActW3, par + kActB3,
               io.packs + (int64_t)k * HKL_PACK_FLOATS, 18, 4};
  float x[S1];
  input_frags(io.obs + row * io.obs_ld, z4(), false, x, q);
  Tile h1, h2;
  gemm_in(an.f1(), x, h1, lane, sfrag);
  gemm256(an.fp(), h1, an.b1, h2, lane, sfrag);
  const f4 pre = gemm_out(an.fo(), h2, an.b2, an.b3, 4, lane, sfrag);
  // the sample's 4 lanes hold the same outputs: lane q stores component q
  const float a = tanh_fast(q == 0 ? pre[0] : q == 1 ? pre[1] : q == 2 ? pre[2] : pre[3]);
  epi(io, row, q, live, a);
}

// Workgroup blockIdx.x's policy k and its rows [start, start + cnt) of the group, 64 per workgroup; false for a
// surplus workgroup.  The result depends on blockIdx and the arguments alone, so a surplus workgroup leaves as a
// whole before the first barrier.
__device__ __forceinline__ bool act_locate(const hkl_act_io &io, int &k, int &start, int &cnt) {
  k = 0, start = 0, cnt = 0;
  if (io.policy) {
    int b = (int)blockIdx.x, lo = io.offsets[0];
    for (k = 0; k < io.n_policies; ++k) {
      const int hi = io.offsets[k + 1], tiles = (hi - lo + 63) >> 6;
      if (b < tiles) {
        start = lo + 64 * b;
        cnt = hi - start;
        break;
      }
      b -= tiles;
      lo = hi;
    }
    if (k == io.n_policies) return false;
  } else {
    start = 64 * (int)blockIdx.x;
    cnt = io.n_rows - start;
  }
  return true;
}

__global__ void __launch_bounds__(WG, 1) act_kernel(hkl_act_io io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];  // two fragment buffers + the staged bias
  int k, start, cnt;
  if (!act_locate(io, k, start, cnt)) return;
  act_tile(io, k, start, cnt, sfrag);
}

// ---- hkl_act_wide: the same acting tile over a bank of up to HKL_ACT_WIDE_MAX_POLICIES policies.  The grouping
// scales with K where hkl_act's 64-entry tables, one-wave scan and per-workgroup walk over the offsets do not:
//   act_wide_zero_kernel     counts := 0;
//   act_wide_hist_kernel     counts[k]: a K-entry histogram per workgroup in LDS, flushed with one global atomic per
//                            (workgroup, occupied k).  A wave whose rows all name one policy adds its row count with
//                            ONE LDS atomic, so a batch on a single policy does not serialise 64 same-address adds
//                            per wave; a batch on all-distinct policies is conflict-free adds and one flush per row;
//   act_wide_scan_kernel     one workgroup: the exclusive scans of the counts (offsets) and of ceil(count / 64) (each
//                            policy's first tile, kept in LDS), counts := 0, counts[K] = the number of tiles, and the
//                            tile table: tile t's (policy, start, rows left) by binary search over the LDS tile scan;
//   act_wide_scatter_kernel  order, as act_scatter_kernel writes it;
//   act_wide_kernel          workgroup b reads tile b of the table: no walk, no search.
// Ids outside [0, K) never index a table (act_policy's guard), and what the kernels read back from their own scratch
// is range-checked before it addresses anything.
constexpr int kWideK = HKL_ACT_WIDE_MAX_POLICIES;

__device__ __forceinline__ int act_wide_policy(const hkl_act_wide_io &io, int i) {
  const int k = io.policy[i];
  return (k >= 0 && k < io.n_policies) ? k : -1;
}

__device__ __forceinline__ int act_wide_max_tiles(const hkl_act_wide_io &io) {
  const int64_t t = (int64_t)((io.n_rows + 63) / 64) + io.n_policies;
  return (int)(t < io.n_rows ? t : io.n_rows);
}

// h[k] += 1 for this lane's policy (k < 0: none); returns the lane's rank among the workgroup's rows of k so far.
// A wave on one policy issues a single LDS atomic.
__device__ __forceinline__ int act_wide_count(int *h, int k) {
  const int lane = threadIdx.x & 63;
  const uint64_t acting = __ballot(k >= 0);
  if (!acting) return 0;
  const int first = __ffsll((unsigned long long)acting) - 1;
  const int k0 = __shfl(k, first);
  if (!__ballot(k >= 0 && k != k0)) {
    int base = 0;
    if (lane == first) base = atomicAdd(&h[k0], __popcll(acting));
    base = __shfl(base, first);
    return base + __popcll(acting & ((1ull << lane) - 1ull));
  }
  return k >= 0 ? atomicAdd(&h[k], 1) : 0;
}

// counts[0 .. K] := 0.  A kernel, not a memset node: the five steps then replay from a captured graph as five kernel
// nodes in a line
__global__ void __launch_bounds__(256) act_wide_zero_kernel(hkl_act_wide_io io) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e <= io.n_policies) io.counts[e] = 0;
}

__global__ void __launch_bounds__(256) act_wide_hist_kernel(hkl_act_wide_io io) {
  __shared__ int h[kWideK];
  for (int e = threadIdx.x; e < io.n_policies; e += 256) h[e] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  act_wide_count(h, i < io.n_rows ? act_wide_policy(io, i) : -1);
  __syncthreads();
  for (int e = threadIdx.x; e < io.n_policies; e += 256)
    if (h[e]) atomicAdd(&io.counts[e], h[e]);
}

__global__ void __launch_bounds__(256) act_wide_scan_kernel(hkl_act_wide_io io) {
  __shared__ int s_off[kWideK + 1], s_tile[kWideK + 1], wrows[4], wtiles[4];
  const int K = io.n_policies, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (K + 255) >> 8, k0 = tid * per;  // this thread's policies [k0, k0 + per), per <= 16
  int rows = 0, tl = 0;
  for (int e = 0; e < per; ++e) {
    const int kk = k0 + e;
    int c = kk < K ? io.counts[kk] : 0;
    c = c < 0 ? 0 : c > io.n_rows ? io.n_rows : c;
    rows += c;
    tl += (c + 63) >> 6;
  }
  int sr = rows, stl = tl;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_up(sr, d), b = __shfl_up(stl, d);
    if (lane >= d) {
      sr += a;
      stl += b;
    }
  }
  if (lane == 63) {
    wrows[wave] = sr;
    wtiles[wave] = stl;
  }
  __syncthreads();
  int run_r = sr - rows, run_t = stl - tl;
  for (int w = 0; w < wave; ++w) {
    run_r += wrows[w];
    run_t += wtiles[w];
  }
  for (int e = 0; e < per; ++e) {
    const int kk = k0 + e;
    if (kk >= K) break;
    int c = io.counts[kk];
    c = c < 0 ? 0 : c > io.n_rows ? io.n_rows : c;
    s_off[kk] = run_r;
    s_tile[kk] = run_t;
    io.offsets[kk] = run_r;
    io.counts[kk] = 0;  // the scatter's cursors
    run_r += c;
    run_t += (c + 63) >> 6;
  }
  const int max_tiles = act_wide_max_tiles(io);
  if (tid == 255) {  // its policies end at or past K: the running values are the totals
    s_off[K] = run_r;
    s_tile[K] = run_t;
    io.offsets[K] = run_r;
    io.counts[K] = run_t < max_tiles ? run_t : max_tiles;
  }
  __syncthreads();
  const int n_tiles = s_tile[K] < max_tiles ? s_tile[K] : max_tiles;
  for (int t = tid; t < n_tiles; t += 256) {
    int lo = 0, hi = K;  // s_tile[lo] <= t < s_tile[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_tile[mid] > t) hi = mid;
      else lo = mid;
    }
    const int start = s_off[lo] + 64 * (t - s_tile[lo]);
    int *tab = io.tiles + 3 * (int64_t)t;
    tab[0] = lo;
    tab[1] = start;
    tab[2] = s_off[lo + 1] - start;
  }
}

__global__ void __launch_bounds__(256) act_wide_scatter_kernel(hkl_act_wide_io io) {
  __shared__ int h[kWideK];  // the workgroup's rows per policy, then the base of its range in the policy's group
  for (int e = threadIdx.x; e < io.n_policies; e += 256) h[e] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int k = i < io.n_rows ? act_wide_policy(io, i) : -1;
  const int rank = act_wide_count(h, k);
  __syncthreads();
  for (int e = threadIdx.x; e < io.n_policies; e += 256)
    if (h[e]) h[e] = io.offsets[e] + atomicAdd(&io.counts[e], h[e]);
  __syncthreads();
  if (k >= 0) {
    const int p = h[k] + rank;  // < offsets[k + 1] <= n_rows: the hist pass counted the same rows
    if (p >= 0 && p < io.n_rows) io.order[p] = i;
  }
}

__global__ void __launch_bounds__(WG, 1) act_wide_kernel(hkl_act_wide_io io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];
  // everything up to act_tile depends on blockIdx, the arguments and the table alone: a surplus workgroup leaves as
  // a whole before the first barrier
  int k = 0, start = 0, cnt = 0;
  if (io.policy) {
    const int b = (int)blockIdx.x;
    if (b >= io.counts[io.n_policies]) return;
    const int *tab = io.tiles + 3 * (int64_t)b;
    k = tab[0];
    start = tab[1];
    cnt = tab[2];
    if (k < 0 || k >= io.n_policies || start < 0 || cnt <= 0 || start > io.n_rows - (cnt < 64 ? cnt : 64)) return;
  } else {
    start = 64 * (int)blockIdx.x;
    cnt = io.n_rows - start;
  }
  act_tile(io, k, start, cnt, sfrag);
}

}  // namespace hkl
