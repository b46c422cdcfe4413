// hkl_per.h -- prioritized replay (rl/replay/prioritized_buffer.py) on per-block sums, for hk_learner.hip; uses
// philox (hkl_rng.h) and sample_noise of hkl_td3.h.
//
// PrioritizedRing.sample_indices is searchsorted(cumsum(p), u * sum(p), right) over all `cap` slots, with p the
// sanitised weights (include/hockey_learner.h).  Here the ring is cut into blocks of PER_BLOCK = 64 x PER_SUB
// consecutive slots and a float64 sum per block is kept current, so that a draw reads the block prefix and ONE
// block, a priority write-back recomputes the blocks it touched, and a push the blocks it covers: none of them
// depends on the ring's capacity beyond the prefix over cap / 1024 block sums.
//
// Fixed orders (no floating-point atomics anywhere, so the same inputs give the same bits on every run and replay):
//   * a block is read by one wave, lane l holding the sub-chunk of slots 16 l .. 16 l + 15: its sum c_l is taken
//     slot by slot, the lane prefix S_l = (..(c_0 + c_1) + ..) + c_l lane by lane, and bsum = S_63; the refresh and
//     the draw share this code (per_scan), so a draw sees exactly the sums that were stored;
//   * the block prefix bpre is one workgroup's scan: 16 waves over contiguous segments, a Kogge-Stone scan per 64
//     entries, carried along the segment, then the segments' offsets added in segment order.
// A draw takes t = u * bpre[last], searches bpre for the first block b with bpre[b] > t, then the first lane with
// bpre[b - 1] + S_l > t and in it the first slot with (bpre[b - 1] + S_{l-1}) + r_k > t (r_k the running sum inside
// the sub-chunk).  When every sum is exact (the tests' dyadic weights) this IS the searchsorted over the full cumsum;
// otherwise the levels associate differently by a few ulps of the total, far inside the summation error of any
// float64 cumsum over the ring, and a level that finds no crossing falls to its last entry (clamped to *size - 1).
#pragma once
#include "hkl_td3.h"

namespace hkl {

constexpr int PER_BLOCK = HKL_PER_BLOCK;
constexpr int PER_SUB = PER_BLOCK / 64;  // slots per lane
static_assert(PER_SUB == 16, "per_load reads a lane's sub-chunk as four float4");

__device__ __forceinline__ double per_weight(float w) {  // max(nan_to_num(w, 0, 0, 0), 1e-6f)
  return (double)((w > 1e-6f && w <= 3.4028234663852886e38f) ? w : 1e-6f);
}
__device__ __forceinline__ float nan_max(float m, float a) { return (a > m || a != a) ? a : m; }  // torch.max: NaN wins
__device__ __forceinline__ float wave_nan_max(float m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = nan_max(m, __shfl_xor(m, d));
  return m;
}
__device__ __forceinline__ int64_t per_size(const hkl_per &P, int64_t size_arg) {
  int64_t s = size_arg >= 0 ? size_arg : *P.size;
  return s < 0 ? 0 : (s > P.cap ? P.cap : s);
}

// this lane's sub-chunk of block blk: r[k] = the running sum of p over its first k + 1 slots; returns the maximum of
// its raw weights inside the ring
__device__ __forceinline__ float per_load(const hkl_per &P, int64_t blk, int lane, int64_t size, double (&r)[PER_SUB]) {
  const int64_t base = blk * PER_BLOCK + (int64_t)lane * PER_SUB;
  float w[PER_SUB];
  if (base + PER_SUB <= P.cap) {
#pragma unroll
    for (int q = 0; q < PER_SUB / 4; ++q) {
      const f4 v = *reinterpret_cast<const f4 *>(P.w + base + 4 * q);
      w[4 * q] = v[0], w[4 * q + 1] = v[1], w[4 * q + 2] = v[2], w[4 * q + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER_SUB; ++k) w[k] = base + k < P.cap ? P.w[base + k] : 0.0f;
  }
  float mx = -__builtin_inff();
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < PER_SUB; ++k) {
    if (base + k < P.cap) mx = nan_max(mx, w[k]);
    run += base + k < size ? per_weight(w[k]) : 0.0;
    r[k] = run;
  }
  return mx;
}
// S_lane = ((c_0 + c_1) + ...) + c_lane, every lane running the same chain
__device__ __forceinline__ double per_lane_prefix(double c, int lane) {
  double run = 0.0, s = 0.0;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    run += __shfl(c, j);
    if (j == lane) s = run;
  }
  return s;
}
// one wave: recompute bsum / bmax of block blk
__device__ __forceinline__ void per_block_refresh(const hkl_per &P, int64_t blk, int lane, int64_t size) {
  double r[PER_SUB];
  const float mx = wave_nan_max(per_load(P, blk, lane, size, r));
  const double s = per_lane_prefix(r[PER_SUB - 1], lane);
  if (lane == 63) P.bsum[blk] = s;
  if (lane == 0) P.bmax[blk] = mx;
}

// The bodies below follow the learner kernels' rule (sample_body): a __device__ function of the member's struct, called
// by the single-member kernel on its by-value argument and by the *_group_kernel on member blockIdx.y's struct in device
// memory.  No body reads blockIdx.y, so member m computes what the single call computes, in the same order.

// blocks b0 .. b0 + nb - 1, one wave each
__global__ void __launch_bounds__(256) per_refresh_kernel(hkl_per P, int64_t b0, int64_t nb, int64_t size_arg) {
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= nb) return;
  per_block_refresh(P, b0 + v, threadIdx.x & 63, per_size(P, size_arg));
}
// every block of every member (equal cap: nblk blocks each)
__global__ void __launch_bounds__(256) per_refresh_group_kernel(const hkl_per *__restrict__ pers, int64_t nblk) {
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= nblk) return;
  const hkl_per &P = pers[blockIdx.y];
  per_block_refresh(P, v, threadIdx.x & 63, per_size(P, -1));
}

// bpre = inclusive prefix of bsum: one workgroup of 16 waves; a wave fetches eight rounds of 64 entries at a time (the
// loads, not the additions, bound this kernel) and scans them in order
__device__ __forceinline__ void per_prefix_body(const hkl_per &P, int64_t nblk) {
  __shared__ double tot[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t seg = ((nblk + 16 * 64 - 1) / (16 * 64)) * 64;  // entries per wave, a multiple of 64
  const int64_t lo = wv * seg, hi = lo + seg < nblk ? lo + seg : nblk;
  double carry = 0.0;
  for (int64_t i0 = lo; i0 < hi; i0 += 64 * 8) {
    double xs[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t i = i0 + q * 64 + lane;
      xs[q] = i < hi ? P.bsum[i] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {  // a round past the segment's end adds zeros: the carry passes through
      const int64_t i = i0 + q * 64 + lane;
      double x = xs[q];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const double y = __shfl_up(x, d);
        if (lane >= d) x += y;
      }
      x += carry;
      if (i < hi) P.bpre[i] = x;
      carry = __shfl(x, 63);
    }
  }
  if (lane == 0) tot[wv] = carry;
  __syncthreads();
  double off = 0.0;
  for (int j = 0; j < wv; ++j) off += tot[j];
  if (wv == 0) return;
  for (int64_t i0 = lo; i0 < hi; i0 += 64 * 8) {
    double xs[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t i = i0 + q * 64 + lane;
      xs[q] = i < hi ? P.bpre[i] : 0.0;  // written above by this same thread
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t i = i0 + q * 64 + lane;
      if (i < hi) P.bpre[i] = off + xs[q];
    }
  }
}
__global__ void __launch_bounds__(1024) per_prefix_kernel(hkl_per P, int64_t nblk) { per_prefix_body(P, nblk); }
__global__ void __launch_bounds__(1024) per_prefix_group_kernel(const hkl_per_sample_io *__restrict__ ios, int64_t nblk) {
  per_prefix_body(ios[blockIdx.y].per, nblk);
}

// one wave per sample
__device__ __forceinline__ void per_sample_body(const hkl_per_sample_io &io, int64_t nblk) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= io.batch) return;
  const hkl_per &P = io.per;
  const int64_t size = per_size(P, -1);
  const uint64_t ctr = io.counter ? (uint64_t)*io.counter : 0;
  double u;
  if (io.u) {
    u = io.u[e];
  } else {  // sample_slot's draw
    const P4 r0 = philox(io.seed, P4{(uint32_t)e, (uint32_t)(e >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32)});
    const uint64_t bits = (((uint64_t)r0.x << 32) | r0.y) >> 11;
    u = (double)bits * (1.0 / 9007199254740992.0);
  }
  const double t = u * P.bpre[nblk - 1];
  // the first block with bpre > t (the last block if there is none), in two rounds of parallel loads instead of a
  // bisection's chain: the first group of 64 blocks whose last entry exceeds t, then the first such entry in it
  const int64_t ngrp = (nblk + 63) / 64;
  int64_t gfirst = ngrp;
  for (int64_t g0 = 0; g0 < ngrp; g0 += 64 * 8) {
    double c[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t g = g0 + q * 64 + lane, i = g * 64 + 63;
      c[q] = g < ngrp ? P.bpre[i < nblk ? i : nblk - 1] : 0.0;
    }
#pragma unroll
    for (int q = 7; q >= 0; --q) {
      const int64_t g = g0 + q * 64 + lane;
      if (g < ngrp && c[q] > t) gfirst = g;
    }
    if (__ballot(gfirst < ngrp)) break;  // later rounds hold later groups
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t o = __shfl_xor((long long)gfirst, d);
    gfirst = o < gfirst ? o : gfirst;
  }
  int64_t b = nblk - 1;
  if (gfirst < ngrp) {
    const int64_t i = gfirst * 64 + lane;
    const uint64_t over = __ballot(i < nblk && P.bpre[i < nblk ? i : nblk - 1] > t);
    if (over) b = gfirst * 64 + __ffsll((unsigned long long)over) - 1;
  }
  const double base = b ? P.bpre[b - 1] : 0.0;
  double r[PER_SUB];
  per_load(P, b, lane, size, r);
  const double s = per_lane_prefix(r[PER_SUB - 1], lane);
  double sprev = __shfl_up(s, 1);
  if (lane == 0) sprev = 0.0;
  const uint64_t hit = __ballot(base + s > t);
  const int ls = hit ? __ffsll((unsigned long long)hit) - 1 : 63;
  const double bl = base + sprev;
  int k = PER_SUB - 1;
#pragma unroll
  for (int kk = PER_SUB - 1; kk >= 0; --kk)
    if (bl + r[kk] > t) k = kk;
  k = __shfl(k, ls);
  int64_t slot = b * PER_BLOCK + (int64_t)ls * PER_SUB + k;
  if (slot > size - 1) slot = size - 1;
  if (slot < 0) slot = 0;
  if (lane == 0) {
    io.idx[e] = slot;
    if (io.noise) *reinterpret_cast<f4 *>(io.noise + e * 4) = sample_noise(io.seed, e, ctr, io.scale, io.clip);
  }
}
__global__ void __launch_bounds__(256) per_sample_kernel(hkl_per_sample_io io, int64_t nblk) { per_sample_body(io, nblk); }
__global__ void __launch_bounds__(256) per_sample_group_kernel(const hkl_per_sample_io *__restrict__ ios, int64_t nblk) {
  per_sample_body(ios[blockIdx.y], nblk);
}

// importance weights of the slots idx[B] (learner.py:199-210), float64 inside.  Every workgroup takes the whole
// batch's sum of raw weights itself -- thread j the samples j, j + 1024, ... in order, the 1024 partials met in a fixed
// tree, so all workgroups hold the same bits -- and the batch's extreme weight: (1 / (p_b size)) ** beta is monotone in
// the weight, so the batch maximum is the same expression at the smallest weight (the largest for beta < 0).  Then
// each writes its own 1024 samples.
__device__ __forceinline__ float per_raw(const hkl_per &P, int64_t s) {
  return P.w[s < 0 ? 0 : (s >= P.cap ? P.cap - 1 : s)];
}
__device__ __forceinline__ void per_iw_body(const hkl_per &P, const int64_t *idx, float *iw, int64_t batch,
                                            double beta) {
  __shared__ double red[1024];
  __shared__ float rmin[1024], rmax[1024];
  const int tid = threadIdx.x;
  const double size = (double)*P.size;
  double acc = 0.0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int64_t e0 = tid; e0 < batch; e0 += 1024 * 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t e = e0 + q * 1024;
      v[q] = e < batch ? per_raw(P, idx[e]) : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (e0 + q * 1024 < batch) {
        acc += (double)v[q];
        mn = v[q] < mn ? v[q] : mn;
        mx = v[q] > mx ? v[q] : mx;
      }
  }
  red[tid] = acc, rmin[tid] = mn, rmax[tid] = mx;
  __syncthreads();
  for (int d = 512; d >= 1; d >>= 1) {
    if (tid < d) {
      red[tid] += red[tid + d];
      rmin[tid] = rmin[tid + d] < rmin[tid] ? rmin[tid + d] : rmin[tid];
      rmax[tid] = rmax[tid + d] > rmax[tid] ? rmax[tid + d] : rmax[tid];
    }
    __syncthreads();
  }
  const double sum = red[0];
  const double top = pow(1.0 / (((double)(beta >= 0.0 ? rmin[0] : rmax[0]) / sum) * size), beta);
  const int64_t e = (int64_t)blockIdx.x * 1024 + tid;
  if (e < batch) iw[e] = (float)(pow(1.0 / (((double)per_raw(P, idx[e]) / sum) * size), beta) / top);
}
__global__ void __launch_bounds__(1024) per_iw_kernel(hkl_per P, const int64_t *idx, float *iw, int64_t batch,
                                                      double beta) {
  per_iw_body(P, idx, iw, batch, beta);
}
// a member without iw takes no weights, as hkl_per_sample launches none for it: its workgroups leave together
__global__ void __launch_bounds__(1024) per_iw_group_kernel(const hkl_per_sample_io *__restrict__ ios) {
  const hkl_per_sample_io &io = ios[blockIdx.y];
  if (!io.iw) return;
  per_iw_body(io.per, io.idx, io.iw, io.batch, io.beta);
}

// write-back, pass 1: the last position of every slot (and one position per touched block) by integer maxima
__device__ __forceinline__ void per_mark_body(const hkl_per_update_io &io) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= io.batch) return;
  const int64_t s = io.idx[e];
  if (s < 0 || s >= io.per.cap) return;
  atomicMax(io.per.last + s, (int)e + 1);
  atomicMax(io.per.bown + s / PER_BLOCK, (int)e + 1);
}
__global__ void __launch_bounds__(256) per_mark_kernel(hkl_per_update_io io) { per_mark_body(io); }
__global__ void __launch_bounds__(256) per_mark_group_kernel(const hkl_per_update_io *__restrict__ ios) {
  per_mark_body(ios[blockIdx.y]);
}
// pass 2: only a slot's last position writes, and clears the slot's word
__device__ __forceinline__ void per_write_body(const hkl_per_update_io &io) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= io.batch) return;
  const int64_t s = io.idx[e];
  if (s < 0 || s >= io.per.cap) return;
  if (__hip_atomic_load(io.per.last + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (int)e + 1) return;
  const float td = io.td[e];
  io.per.w[s] = td < 1e-6f ? 1e-6f : (td > 1e6f ? 1e6f : td);  // NaN stays, as np.clip
  __hip_atomic_store(io.per.last + s, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void __launch_bounds__(256) per_write_kernel(hkl_per_update_io io) { per_write_body(io); }
__global__ void __launch_bounds__(256) per_write_group_kernel(const hkl_per_update_io *__restrict__ ios) {
  per_write_body(ios[blockIdx.y]);
}
// pass 3: one wave per position; the one a touched block recorded recomputes it and clears the block's word
__device__ __forceinline__ void per_touch_body(const hkl_per_update_io &io) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= io.batch) return;
  const int64_t s = io.idx[e];
  if (s < 0 || s >= io.per.cap) return;
  const int64_t blk = s / PER_BLOCK;
  if (__hip_atomic_load(io.per.bown + blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (int)e + 1) return;
  per_block_refresh(io.per, blk, threadIdx.x & 63, per_size(io.per, -1));
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(io.per.bown + blk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void __launch_bounds__(256) per_touch_kernel(hkl_per_update_io io) { per_touch_body(io); }
__global__ void __launch_bounds__(256) per_touch_group_kernel(const hkl_per_update_io *__restrict__ ios) {
  per_touch_body(ios[blockIdx.y]);
}

// PrioritizedRing._before_push: max(w[0 : size_after]) from bmax over the full blocks and a scan of the ragged one,
// stored to the n pushed slots
__device__ __forceinline__ void per_push_body(const hkl_per &P, int64_t pos, int64_t n, int64_t size_after) {
  __shared__ float red[1024];
  const int tid = threadIdx.x;
  const int64_t nfull = size_after / PER_BLOCK;
  float m = -__builtin_inff();
  for (int64_t b = tid; b < nfull; b += 1024) m = nan_max(m, P.bmax[b]);
  for (int64_t i = nfull * PER_BLOCK + tid; i < size_after; i += 1024) m = nan_max(m, P.w[i]);
  red[tid] = m;
  __syncthreads();
  for (int d = 512; d >= 1; d >>= 1) {
    if (tid < d) red[tid] = nan_max(red[tid], red[tid + d]);
    __syncthreads();
  }
  const float top = red[0];  // every read of w above precedes the barriers
  for (int64_t j = tid; j < n; j += 1024) {
    int64_t s = pos + j;
    if (s >= P.cap) s -= P.cap;
    P.w[s] = top;
  }
}
__global__ void __launch_bounds__(1024) per_push_kernel(hkl_per P, int64_t pos, int64_t n, int64_t size_after) {
  per_push_body(P, pos, n, size_after);
}

// The grouped push reads member m's (pos, n, size_after) from device memory.  What the host checks in hkl_per_push is
// the caller's contract here; values outside it are made harmless on the device instead: a count is cut to
// [0, max_n] (max_n <= cap), the fill level to [0, cap], and a member whose pos lies outside the ring is skipped, so
// that no store or load leaves the member's arrays whatever the three arrays hold.
struct PushArgs {
  int64_t pos, n, size_after;
};
__device__ __forceinline__ PushArgs per_push_args(const hkl_per &P, const int64_t *pos, const int64_t *n,
                                                  const int64_t *size_after, int64_t max_n) {
  const int m = blockIdx.y;
  PushArgs a{pos[m], n[m], size_after[m]};
  a.n = a.n > max_n ? max_n : a.n;
  if (a.pos < 0 || a.pos >= P.cap) a.n = 0;
  a.size_after = a.size_after < 0 ? 0 : (a.size_after > P.cap ? P.cap : a.size_after);
  return a;
}
__global__ void __launch_bounds__(1024) per_push_group_kernel(const hkl_per *__restrict__ pers, const int64_t *pos,
                                                              const int64_t *n, const int64_t *size_after,
                                                              int64_t max_n) {
  const hkl_per &P = pers[blockIdx.y];
  const PushArgs a = per_push_args(P, pos, n, size_after, max_n);
  if (a.n <= 0) return;  // the whole workgroup: nothing is stored for this member
  per_push_body(P, a.pos, a.n, a.size_after);
}
// hkl_per_push's two refreshes in one grid: waves [0, n_head) take the blocks of the head slots pos .. pos + head - 1,
// waves [n_head, n_head + n_tail) those of the wrapped tail 0 .. n - head - 1; n_head / n_tail are the host's bounds
// for a push of max_n slots, and a wave past its member's own ranges exits.
__global__ void __launch_bounds__(256) per_push_refresh_group_kernel(const hkl_per *__restrict__ pers,
                                                                     const int64_t *pos, const int64_t *n,
                                                                     const int64_t *size_after, int64_t max_n,
                                                                     int64_t n_head, int64_t n_tail) {
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n_head + n_tail) return;
  const hkl_per &P = pers[blockIdx.y];
  const PushArgs a = per_push_args(P, pos, n, size_after, max_n);
  if (a.n <= 0) return;
  const int64_t head = P.cap - a.pos < a.n ? P.cap - a.pos : a.n;
  int64_t blk;
  if (v < n_head) {
    const int64_t b0 = a.pos / PER_BLOCK;
    blk = b0 + v;
    if (blk > (a.pos + head - 1) / PER_BLOCK) return;
  } else {
    blk = v - n_head;
    if (head >= a.n || blk > (a.n - head - 1) / PER_BLOCK) return;
  }
  per_block_refresh(P, blk, threadIdx.x & 63, per_size(P, a.size_after));
}

}  // namespace hkl
