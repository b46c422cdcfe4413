// hk_learner.hip -- the batched TD3 learner (BASELINE C5) as fused fp32 MFMA kernels for gfx950.
//
// One learner update of rl/td3/learner.py:55-218 at a large batch B (C5 draws 16 384 samples per update):
//   critic_step   target policy smoothing + clipped double-Q target (compute_target, :75-112), both critics'
//                 forward, the weighted smooth-L1 loss (rl/utils/torch_utils.py:12-24) and its backward through
//                 both critics down to the first layer -- one launch, B / 64 workgroups of 4 waves, 16 samples
//                 per wave;
//   actor_step    actor forward, Q1 of the updated critic on (s, actor(s)), -mean Q1 backward through Q1 to the
//                 action and through the actor (update_actor, :138-175) -- one launch;
//   wgrad         the weight gradients dW = dZ^T X (the reduction over the batch) as split-K MFMA tiles;
//   adam          per-parameter reduction of the gradient slabs in a fixed order + torch.optim.Adam's update
//                 (lr, betas (0.9, 0.999), eps, L2 weight decay; rl/td3/agent.py:174-182), on actor updates with
//                 soft_update (:196-218) folded in;
//   pack          re-lays the changed weights out for the MFMA operands (polyak: soft_update as its own launch).
//   per_*         prioritized replay on per-block float64 sums: slots, importance weights, the priority write-back and
//                 the push rule without a pass over the ring (after the C ABI of the stages above); their *_group
//                 forms run up to 64 rings per launch, the push with its sizes read on the device.
//   act           acting: the actor forward of actor_step over a bank of policies, a different one per row, the rows
//                 grouped by policy on the device (near the end of this file).
//   value         twin-critic inference: Q_k(s, a), or V(s) = min Q_k(s, actor(s)) with the action kept in registers
//                 (the last section of this file).
//
// Every product is v_mfma_f32_16x16x4_f32: exact f32 fma chains (no reduced-precision path on gfx950), so the
// arithmetic is the reference's fp32 up to summation order.  Layout of a wave's activations ("Tile"): lane l holds
// sample j = l & 15 and, for each 16-neuron block ob and r = 0..3, neuron 16 ob + 4 (l >> 4) + r in v[ob][r] --
// exactly the C/D layout of the MFMA (col = lane & 15, row = 4 (lane >> 4) + reg), and, read as a B operand with
// k-step (kb, r), exactly the fragment the next layer needs (lane (j, kk = l >> 4) holds input neuron
// 16 kb + 4 kk + r).  Consecutive layers therefore chain in registers with no data movement; the weights are
// pre-packed into the matching A-operand order (pack_kernel) after every optimiser step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hockey_learner.h"

namespace hkl {

constexpr int H = 256;   // hidden width (rl/td3/networks.py: h = 256)
constexpr int XP = 32;   // padded row of the stored first-layer inputs X0 [B][XP]
constexpr int S1 = 6;    // first-layer k-steps: inputs padded to 24
constexpr int WG = 256;  // threads of the fused kernels: 4 waves x 16 samples = 64 samples per workgroup
constexpr int CHUNK = 256;  // batch granularity; the weight-gradient kernel's split-K chunks are 256 or 512 samples

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f4 z4() { return f4{0.0f, 0.0f, 0.0f, 0.0f}; }

struct Tile {
  f4 v[16];
};

// tanh without branches: tanh|x| = (1 - t) / (1 + t), t = 2^(-2 log2(e) |x|) (v_exp_f32, v_rcp_f32), sign restored.
// OCML's tanhf branches between a polynomial and an exp path per lane (exec-mask juggling around ~30 VALU per
// call, a third of the critic kernel's instructions); this form is 7 VALU.  Its absolute error is a few 1e-8 near
// 0 (the 1 - t cancellation) and below 2e-7 everywhere (checked against torch.tanh in
// tests/test_gpu_learner.py), far inside the learner's stated fp32 tolerances.
__device__ __forceinline__ float tanh_fast(float x) {
  const float t = __builtin_amdgcn_exp2f(-2.8853900817779268f * fabsf(x));
  const float y = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
  return copysignf(y, x);
}

// ------------------------------------------------------------------------------------------------ packed layouts
// f1 [16 ob][64 lane][8]     : W1[16 ob + (l & 15)][4 s + (l >> 4)] for k-step s < 6 (0 past the input width)
// fp [16 ob][16 kb][64 lane] : f4 over r of W2[16 ob + (l & 15)][16 kb + 4 (l >> 4) + r]        (forward)
// bp [16 ib][16 ob][64 lane] : f4 over r of W2[16 ob + 4 (l >> 4) + r][16 ib + (l & 15)]        (W2^T: backward)
// fo [16 kb][64 lane]        : f4 over r of W3[l & 15][16 kb + 4 (l >> 4) + r] (0 for rows >= n_out)
// wa [256]                   : f4 of W1[n][18..21] (a critic's action columns: dQ/da)
constexpr int kF1 = 16 * 64 * 8, kFp = 16 * 16 * 64 * 4, kBp = kFp, kFo = 16 * 64 * 4, kWa = 256 * 4;
constexpr int kPackFloats = kF1 + kFp + kBp + kFo + kWa;
static_assert(kPackFloats == HKL_PACK_FLOATS, "pack size (include/hockey_learner.h)");

struct Net {  // device view of one MLP (n_in -> 256 -> 256 -> n_out)
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const float *pk;
  int n_in, n_out;
  __device__ const float *f1() const { return pk; }
  __device__ const f4 *fp() const { return reinterpret_cast<const f4 *>(pk + kF1); }
  __device__ const f4 *bp() const { return reinterpret_cast<const f4 *>(pk + kF1 + kFp); }
  __device__ const f4 *fo() const { return reinterpret_cast<const f4 *>(pk + kF1 + kFp + kBp); }
  __device__ const f4 *wa() const { return reinterpret_cast<const f4 *>(pk + kF1 + kFp + kBp + kFo); }
};
__host__ __device__ inline Net net_of(const hkl_net &n) { return Net{n.w1, n.b1, n.w2, n.b2, n.w3, n.b3, n.pack, n.n_in, n.n_out}; }

// ------------------------------------------------------------------------------------------------ layer routines
// out = W1 x (no bias): x[s] = this lane's input for k-step s (feature 4 s + (lane >> 4)).  Workgroup-collective:
// the 32 KB first-layer pack is staged in LDS (both fragment buffers) once for the 4 waves.
__device__ __forceinline__ void gemm_in(const float *__restrict__ f1, const float (&x)[S1], Tile &out, int lane,
                                        f4 *sfrag) {
  const f4 *src = reinterpret_cast<const f4 *>(f1);
#pragma unroll
  for (int i = 0; i < 8; ++i) sfrag[threadIdx.x + i * WG] = src[threadIdx.x + i * WG];
  __syncthreads();
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) {
    const f4 lo = sfrag[(ob * 64 + lane) * 2];
    const f4 hi = sfrag[(ob * 64 + lane) * 2 + 1];
    f4 acc = z4();
    acc = mfma(lo[0], x[0], acc);
    acc = mfma(lo[1], x[1], acc);
    acc = mfma(lo[2], x[2], acc);
    acc = mfma(lo[3], x[3], acc);
    acc = mfma(hi[0], x[4], acc);
    acc = mfma(hi[1], x[5], acc);
    out.v[ob] = acc;
  }
  __syncthreads();  // the staging buffers are reused by the next collective call
}

// out = P in, P a packed 256 x 256 operand (fp: W2 in; bp: W2^T in), a workgroup-collective call (all 4 waves).
// The A fragments are the same for the workgroup's 4 waves: each 16-neuron k-block (16 KB) is loaded once per
// workgroup into one of two LDS buffers (each thread 4 x 16 B) while the waves multiply the previous one, so the
// L2 serves a quarter of the bytes.  bias != nullptr: `in` holds pre-activations and block kb is activated in
// place (tanh(in + bias)) just before its first use, so the activation's VALU work overlaps the MFMAs of the
// block before; on return `in` holds the activations.
__device__ __forceinline__ void gemm256(const f4 *__restrict__ P, Tile &in, const float *__restrict__ bias, Tile &out,
                                        int lane, f4 *sfrag) {
  const int wave = threadIdx.x >> 6, q = lane >> 4;
  float *sbias = reinterpret_cast<float *>(sfrag + 2 * 1024);  // the bias, staged once (no global wait per k-block)
  if (bias) sbias[threadIdx.x] = bias[threadIdx.x];
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) out.v[ob] = z4();
  f4 g[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) g[i] = P[((4 * wave + i) * 16) * 64 + lane];
#pragma unroll
  for (int i = 0; i < 4; ++i) sfrag[(4 * wave + i) * 64 + lane] = g[i];
  __syncthreads();
#pragma unroll
  for (int kb = 0; kb < 16; ++kb) {
    const f4 *buf = sfrag + (kb & 1) * 1024;
    if (kb + 1 < 16) {
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i] = P[((4 * wave + i) * 16 + kb + 1) * 64 + lane];
    }
    f4 a[16];
#pragma unroll
    for (int ob = 0; ob < 16; ++ob) a[ob] = buf[ob * 64 + lane];
    if (bias) {
      const f4 bb = *reinterpret_cast<const f4 *>(sbias + 16 * kb + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) in.v[kb][r] = tanh_fast(in.v[kb][r] + bb[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float b = in.v[kb][r];
#pragma unroll
      for (int ob = 0; ob < 16; ++ob) out.v[ob] = mfma(a[ob][r], b, out.v[ob]);
    }
    if (kb + 1 < 16) {
      f4 *nb = sfrag + ((kb + 1) & 1) * 1024;
#pragma unroll
      for (int i = 0; i < 4; ++i) nb[(4 * wave + i) * 64 + lane] = g[i];
    }
    __syncthreads();
  }
}

// t = tanh(t + b) (Linear bias, then the tanh activation)
__device__ __forceinline__ void bias_tanh(Tile &t, const float *__restrict__ b, int q) {
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) {
    const f4 bb = *reinterpret_cast<const f4 *>(b + 16 * ob + 4 * q);
#pragma unroll
    for (int r = 0; r < 4; ++r) t.v[ob][r] = tanh_fast(t.v[ob][r] + bb[r]);
  }
}

// the n_out (<= 4) outputs W3 h + b3 of this lane's sample, broadcast to every lane of the sample; a
// workgroup-collective call (the W3 fragments and the bias are staged in LDS once for the 4 waves).  bias !=
// nullptr: h holds pre-activations, activated in place (tanh(h + bias)) block by block as in gemm256.
__device__ __forceinline__ f4 gemm_out(const f4 *__restrict__ fo, Tile &h, const float *__restrict__ bias,
                                       const float *__restrict__ b3, int n_out, int lane, f4 *sfrag) {
  const int q = lane >> 4;
  float *sbias = reinterpret_cast<float *>(sfrag + 2 * 1024);
#pragma unroll
  for (int i = 0; i < 4; ++i) sfrag[threadIdx.x + i * WG] = fo[threadIdx.x + i * WG];
  if (bias) sbias[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  f4 acc0 = z4(), acc1 = z4();
#pragma unroll
  for (int kb = 0; kb < 16; ++kb) {
    const f4 a = sfrag[kb * 64 + lane];
    if (bias) {
      const f4 bb = *reinterpret_cast<const f4 *>(sbias + 16 * kb + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) h.v[kb][r] = tanh_fast(h.v[kb][r] + bb[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (kb & 1) acc1 = mfma(a[r], h.v[kb][r], acc1);
      else acc0 = mfma(a[r], h.v[kb][r], acc0);
    }
  }
  __syncthreads();  // the staging buffers are reused by the next collective call
  const f4 acc = acc0 + acc1;  // lanes 0..15 hold outputs 0..3 of sample lane & 15
  f4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = __shfl(acc[r], lane & 15) + (r < n_out ? b3[r] : 0.0f);
  return o;
}

// A one-output head (a critic's Q): W3[0] . tanh(h + bias) + b3[0] for this lane's sample, returned to every lane of
// the sample, h activated in place as gemm_out leaves it.  VALU dot products (each lane's 64 neurons, four partial
// sums) and two cross-row shuffles instead of a 16 x 16 MFMA tile of which one row is used; no LDS staging and no
// workgroup barrier.  The 4 lanes of a sample add the same partials in commuted order, so they agree bit for bit.
__device__ __forceinline__ float head1(const float *__restrict__ w3, Tile &h, const float *__restrict__ bias,
                                       const float *__restrict__ b3, int lane) {
  const int q = lane >> 4;
  f4 acc = z4();
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) {
    const f4 bb = *reinterpret_cast<const f4 *>(bias + 16 * ob + 4 * q);
    const f4 w = *reinterpret_cast<const f4 *>(w3 + 16 * ob + 4 * q);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h.v[ob][r] = tanh_fast(h.v[ob][r] + bb[r]);
      acc[r] += w[r] * h.v[ob][r];
    }
  }
  float v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v + b3[0];
}

// dh = W3^T dz3 (dz3: this lane's sample's n_out output gradients)
__device__ __forceinline__ void back_out(const float *__restrict__ w3, int n_out, f4 dz3, Tile &dh, int q) {
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) {
    f4 s = z4();
    for (int o = 0; o < n_out; ++o) {
      const f4 w = *reinterpret_cast<const f4 *>(w3 + o * H + 16 * ob + 4 * q);
      s += w * dz3[o];
    }
    dh.v[ob] = s;
  }
}

// t = t * (1 - y^2): tanh backward (torch tanh_backward: grad * (1 - y * y))
__device__ __forceinline__ void tanh_back(Tile &t, const Tile &y) {
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) t.v[ob] = t.v[ob] * (1.0f - y.v[ob] * y.v[ob]);
}

// sum over the 16 samples of a wave (lanes with equal lane >> 4: one DPP row), every lane of the row gets the sum:
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror -- four v_add with a DPP source
template <int C>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), C, 0xf, 0xf, false));
}
__device__ __forceinline__ float sum16(float v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  v += dpp<0x141>(v);
  v += dpp<0x140>(v);
  return v;
}

__device__ __forceinline__ void store_tile(float *__restrict__ M, const Tile &t, int64_t row, int q) {
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) *reinterpret_cast<f4 *>(M + row * H + 16 * ob + 4 * q) = t.v[ob];
}
__device__ __forceinline__ void load_tile(const float *__restrict__ M, Tile &t, int64_t row, int q) {
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) t.v[ob] = *reinterpret_cast<const f4 *>(M + row * H + 16 * ob + 4 * q);
}

// Workgroup partial of a per-neuron sum over the workgroup's 64 samples: red[w][n] per wave, then the 4 waves in a
// fixed order.  v[ob][r] = this lane's value for neuron 16 ob + 4 q + r (summed over the wave's samples here).
__device__ __forceinline__ void wg_neuron_sum(const Tile &t, float *red, float *__restrict__ out, int wave, int lane) {
  const int q = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < 16; ++ob)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = sum16(t.v[ob][r]);
      if ((lane & 15) == 0) red[wave * H + 16 * ob + 4 * q + r] = s;
    }
  __syncthreads();
  const int n = threadIdx.x;  // WG == H
  out[n] = ((red[n] + red[H + n]) + red[2 * H + n]) + red[3 * H + n];
  __syncthreads();
}
__device__ __forceinline__ float wg_scalar_sum(float v, float *red, int wave, int lane) {
  // v: one value per sample (lanes 0..15 of each wave carry distinct samples; other lanes ignored)
  float s = (lane < 16) ? v : 0.0f;
  s = sum16(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  const float tot = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return tot;
}

// unscale an action in [-1, 1] to the critic's input (TwinQNetwork._unscale_action): ((a - low) / range) * 2 - 1
__device__ __forceinline__ float unscale(float a, float low, float range) { return ((a - low) / range) * 2.0f - 1.0f; }

// first-layer inputs of this lane from a state row (18 features) and 4 action inputs (already unscaled, or 0)
__device__ __forceinline__ void input_frags(const float *__restrict__ srow, const f4 act, bool with_act, float (&x)[S1],
                                            int q) {
#pragma unroll
  for (int s = 0; s < S1; ++s) {
    const int f = 4 * s + q;
    float v = 0.0f;
    if (f < 18) v = srow[f];
    else if (with_act && f < 22) {
      const int c = f - 18;
      v = c == 0 ? act[0] : c == 1 ? act[1] : c == 2 ? act[2] : act[3];
    }
    x[s] = v;
  }
}

// ------------------------------------------------------------------------------------------------ sampling
// The batch's replay slots and target noise from a counter-based RNG (Philox4x32-10 keyed by the learner's seed, the
// counter = (sample, update, purpose)): uniform slots floor(u * size) with a 53-bit u (rl/replay/uniform_buffer.py's
// (rand * size).astype(int)), and the target policy smoothing noise clamp(N(0, scale), -clip, clip) by Box-Muller
// (learner.py:80-93).  The update counter lives in device memory (graph replays advance it): critic_step bumps it.
struct P4 {
  uint32_t x, y, z, w;
};
__device__ __forceinline__ P4 philox(uint64_t key, P4 c) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = P4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// sample e's replay slot of update `ctr` over `size` filled slots.  size <= 0 (an empty ring, or a fill word that is
// out of contract) gives slot 0: out-of-contract device values are clamped, never addressed (as per_sample_body)
__device__ __forceinline__ int64_t sample_slot(uint64_t seed, int64_t e, uint64_t ctr, int64_t size) {
  if (size <= 0) return 0;
  const P4 r0 = philox(seed, P4{(uint32_t)e, (uint32_t)(e >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32)});
  const uint64_t bits = (((uint64_t)r0.x << 32) | r0.y) >> 11;
  const double u = (double)bits * (1.0 / 9007199254740992.0);
  const uint64_t i = (uint64_t)(u * (double)(uint64_t)size);
  return (int64_t)(i < (uint64_t)size ? i : (uint64_t)size - 1);
}
// sample e's clipped target-smoothing noise of update `ctr`
__device__ __forceinline__ f4 sample_noise(uint64_t seed, int64_t e, uint64_t ctr, float scale, float clip) {
  const P4 r1 = philox(seed ^ 0x6E6F697365ull, P4{(uint32_t)e, (uint32_t)(e >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32)});
  const uint32_t w[4] = {r1.x, r1.y, r1.z, r1.w};
  float z[4];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = ((float)(w[2 * p] >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0, 1)
    const float u2 = (float)(w[2 * p + 1] >> 8) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * p] = rad * cs;
    z[2 * p + 1] = rad * sn;
  }
  f4 nz;
#pragma unroll
  for (int c = 0; c < 4; ++c) nz[c] = fminf(fmaxf(z[c] * scale, -clip), clip);
  return nz;
}
// Every learner kernel's body is a __device__ function of its io struct: the single-member kernel passes its by-value
// argument, the grouped twin (the *_group_kernel after it) member m's struct from an array in device memory, m taken
// from a grid dimension the body does not read.  The struct reads are wave-uniform either way.
__device__ __forceinline__ void sample_body(const hkl_sample_io &io) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= io.batch) return;
  const uint64_t ctr = (uint64_t)*io.counter;
  io.idx[e] = sample_slot(io.seed, e, ctr, *io.size);
  *reinterpret_cast<f4 *>(io.noise + e * 4) = sample_noise(io.seed, e, ctr, io.scale, io.clip);
}
__global__ void __launch_bounds__(256) sample_kernel(hkl_sample_io io) { sample_body(io); }
__global__ void __launch_bounds__(256) sample_group_kernel(const hkl_sample_io *__restrict__ ios) {
  sample_body(ios[blockIdx.y]);
}

// ------------------------------------------------------------------------------------------------ critic step
// Q(x) of one critic network (forward only): its output for this lane's sample
__device__ __forceinline__ float q_forward(const Net &c, const float (&x)[S1], Tile &h1, Tile &h2, int lane,
                                           f4 *sfrag) {
  gemm_in(c.f1(), x, h1, lane, sfrag);
  gemm256(c.fp(), h1, c.b1, h2, lane, sfrag);
  return head1(c.w3, h2, c.b2, c.b3, lane);
}

// one critic k of update_critic: forward on x, the weighted smooth-L1 (torch_utils.py:12-24; critic_loss =
// (loss1 + loss2) * 0.5, each a batch mean) and the backward to the first layer.  Stores H1, DZ1, DZ2 for the
// weight gradients (their bias gradients are the column sums wgrad takes); dW3 / db3 as workgroup partials.
__device__ __forceinline__ void critic_one(const hkl_critic_io &io, int k, const Net &c, const float (&x)[S1], float y,
                                           float w, int64_t row, float *red, f4 *sfrag, float &td, float &loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
  Tile h1, h2;
  gemm_in(c.f1(), x, h1, lane, sfrag);
  gemm256(c.fp(), h1, c.b1, h2, lane, sfrag);
  store_tile(io.h1[k], h1, row, q);
  const float qv = head1(c.w3, h2, c.b2, c.b3, lane);
  const float diff = qv - y, ad = fabsf(diff);
  loss += ad < 1.0f ? 0.5f * w * diff * diff : (ad - 0.5f) * w;
  const float g = (ad < 1.0f ? w * diff : (diff > 0.0f ? w : diff < 0.0f ? -w : 0.0f)) * (0.5f / (float)io.batch);
  td += ad;
  // output layer: dW3 = sum_j g_j h2_j, db3 = sum_j g_j
  Tile t;
#pragma unroll
  for (int ob = 0; ob < 16; ++ob) t.v[ob] = h2.v[ob] * g;
  wg_neuron_sum(t, red, io.p_dw3[k] + blockIdx.x * H, wave, lane);
  const float gb = wg_scalar_sum(g, red, wave, lane);
  if (threadIdx.x == 0) io.p_db3[k][blockIdx.x] = gb;
  // dz2 = (W3^T g) * (1 - h2^2)
  back_out(c.w3, 1, f4{g, 0.0f, 0.0f, 0.0f}, t, q);
  tanh_back(t, h2);
  store_tile(io.dz2[k], t, row, q);
  // dz1 = (W2^T dz2) * (1 - h1^2)
  gemm256(c.bp(), t, nullptr, h2, lane, sfrag);
  tanh_back(h2, h1);
  store_tile(io.dz1[k], h2, row, q);
}

// compute_target + update_critic's forward / loss / backward for both critics (learner.py:75-136).
__device__ __forceinline__ void critic_step_body(const hkl_critic_io &io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];  // two fragment buffers + the staged bias
  __shared__ float red[4 * H];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + j;  // this lane's sample (batch row)
  const int64_t src = io.idx[row];                                // its replay slot
  const float *s_row = io.ring_s + src * 18, *s2_row = io.ring_s2 + src * 18;
  const float rwd = io.ring_r[src], dn = io.ring_d[src];
  const f4 act = *reinterpret_cast<const f4 *>(io.ring_a + src * 4);
  const f4 nz = *reinterpret_cast<const f4 *>(io.noise + row * 4);
  const float w = io.iw ? io.iw[row] : 1.0f;
  const Net ta = net_of(io.target_actor), tq[2] = {net_of(io.target_q[0]), net_of(io.target_q[1])};
  const Net cq[2] = {net_of(io.q[0]), net_of(io.q[1])};

  // ---- target: y = r + gamma (1 - d) min(Q1', Q2')(s2, clamp(actor'(s2) + noise, -1, 1))
  float x[S1];
  input_frags(s2_row, z4(), false, x, q);
  Tile h1, h2;
  gemm_in(ta.f1(), x, h1, lane, sfrag);
  gemm256(ta.fp(), h1, ta.b1, h2, lane, sfrag);
  const f4 a2 = gemm_out(ta.fo(), h2, ta.b2, ta.b3, 4, lane, sfrag);
  f4 a2u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float t = fminf(fmaxf(tanh_fast(a2[c]) + nz[c], -1.0f), 1.0f);  // torch.clamp(target_action + noise, -1, 1)
    a2u[c] = unscale(t, io.act_low[c], io.act_range[c]);
  }
  input_frags(s2_row, a2u, true, x, q);
  const float qt0 = q_forward(tq[0], x, h1, h2, lane, sfrag), qt1 = q_forward(tq[1], x, h1, h2, lane, sfrag);
  const float y = rwd + io.gamma * (1.0f - dn) * fminf(qt0, qt1);

  // ---- critics on (s, a)
  f4 au;
#pragma unroll
  for (int c = 0; c < 4; ++c) au[c] = unscale(act[c], io.act_low[c], io.act_range[c]);
  input_frags(s_row, au, true, x, q);
  {  // X0 row (shared by both critics' dW1): 22 features, zero padded; lane q writes 8 of its sample's 32
    float *xr = io.x0 + row * XP;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int f = 8 * q + e;
      xr[f] = f < 18 ? s_row[f] : f < 22 ? au[f - 18] : 0.0f;
    }
  }
  float td = 0.0f, loss = 0.0f;
  critic_one(io, 0, cq[0], x, y, w, row, red, sfrag, td, loss);
  critic_one(io, 1, cq[1], x, y, w, row, red, sfrag, td, loss);
  if (io.td && q == 0) io.td[row] = td * 0.5f;  // (|q1 - y| + |q2 - y|) / 2 (learner.py:163-170)
  const float ls = wg_scalar_sum(loss, red, wave, lane);
  if (threadIdx.x == 0) io.p_loss[blockIdx.x] = ls;
  if (io.sample_counter && blockIdx.x == 0 && threadIdx.x == 0) *io.sample_counter += 1;
}
__global__ void __launch_bounds__(WG, 1) critic_step_kernel(hkl_critic_io io) { critic_step_body(io); }
__global__ void __launch_bounds__(WG, 1) critic_step_group_kernel(const hkl_critic_io *__restrict__ ios) {
  critic_step_body(ios[blockIdx.y]);
}

// ------------------------------------------------------------------------------------------------ actor step
// update_actor's forward / backward (learner.py:138-175): loss = -mean Q1(s, actor(s)) with the updated critic.
__device__ __forceinline__ void actor_step_body(const hkl_actor_io &io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];  // two fragment buffers + the staged bias
  __shared__ float red[4 * H];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + j;
  const int64_t src = io.idx[row];
  const float *s_row = io.ring_s + src * 18;
  const Net an = net_of(io.actor), qn = net_of(io.q1);
  float x[S1];
  input_frags(s_row, z4(), false, x, q);
  {
    float *xr = io.x0 + row * XP;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int f = 8 * q + e;
      xr[f] = f < 18 ? s_row[f] : 0.0f;
    }
  }
  Tile h1, h2;
  gemm_in(an.f1(), x, h1, lane, sfrag);
  gemm256(an.fp(), h1, an.b1, h2, lane, sfrag);
  store_tile(io.h1, h1, row, q);
  const f4 pre = gemm_out(an.fo(), h2, an.b2, an.b3, 4, lane, sfrag);
  store_tile(io.h2, h2, row, q);
  f4 a, au;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    a[c] = tanh_fast(pre[c]);
    au[c] = unscale(a[c], io.act_low[c], io.act_range[c]);
  }
  // Q1(s, a)
  input_frags(s_row, au, true, x, q);
  gemm_in(qn.f1(), x, h1, lane, sfrag);
  gemm256(qn.fp(), h1, qn.b1, h2, lane, sfrag);
  const float qv = gemm_out(qn.fo(), h2, qn.b2, qn.b3, 1, lane, sfrag)[0];
  const float g = -1.0f / (float)io.batch;  // d(-mean q) / dq
  Tile t;
  back_out(qn.w3, 1, f4{g, 0.0f, 0.0f, 0.0f}, t, q);
  tanh_back(t, h2);
  gemm256(qn.bp(), t, nullptr, h2, lane, sfrag);
  tanh_back(h2, h1);  // dz1 of Q1
  // dQ/d(unscaled action) = W1[:, 18:22]^T dz1, summed over the 4 lanes of the sample; then the unscale chain rule
  f4 da = z4();
  const f4 *wa = qn.wa();
#pragma unroll
  for (int ob = 0; ob < 16; ++ob)
#pragma unroll
    for (int r = 0; r < 4; ++r) da += wa[16 * ob + 4 * q + r] * h2.v[ob][r];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float v = da[c];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    da[c] = v * (2.0f / io.act_range[c]);
  }
  // actor output layer: dz3 = da * (1 - a^2); dW3 = sum_j dz3_j h2_j; db3 = sum_j dz3_j
  f4 dz3;
#pragma unroll
  for (int c = 0; c < 4; ++c) dz3[c] = da[c] * (1.0f - a[c] * a[c]);
  load_tile(io.h2, h2, row, q);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int ob = 0; ob < 16; ++ob) t.v[ob] = h2.v[ob] * dz3[c];
    wg_neuron_sum(t, red, io.p_dw3 + ((int64_t)blockIdx.x * 4 + c) * H, wave, lane);
    const float gb = wg_scalar_sum(dz3[c], red, wave, lane);
    if (threadIdx.x == 0) io.p_db3[blockIdx.x * 4 + c] = gb;
  }
  back_out(an.w3, 4, dz3, t, q);
  tanh_back(t, h2);
  store_tile(io.dz2, t, row, q);
  gemm256(an.bp(), t, nullptr, h2, lane, sfrag);
  load_tile(io.h1, h1, row, q);
  tanh_back(h2, h1);
  store_tile(io.dz1, h2, row, q);
  const float ls = wg_scalar_sum(-qv, red, wave, lane);
  if (threadIdx.x == 0) io.p_loss[blockIdx.x] = ls;
}
__global__ void __launch_bounds__(WG, 1) actor_step_kernel(hkl_actor_io io) { actor_step_body(io); }
__global__ void __launch_bounds__(WG, 1) actor_step_group_kernel(const hkl_actor_io *__restrict__ ios) {
  actor_step_body(ios[blockIdx.y]);
}

// ------------------------------------------------------------------------------------------------ weight gradients
// dW[o][k] = sum_j DZ[j][o] X[j][k] over one chunk of CHUNK samples, o in 128-row tiles, k in KT-wide tiles; 4 waves
// as 2 (o) x 2 (k).  The chunk streams through two LDS buffers 32 samples at a time (the next sub-chunk's loads are
// in flight while the current one is multiplied).  Output: slab[chunk][256][ldx] (natural W layout, fp32 partial
// sums; the adam kernel adds the chunks in order).  Blocks of the first k tile also sum DZ's columns: the bias
// gradient partials bslab[chunk][256].  One launch runs up to 4 jobs (blockIdx.z = job * chunks + chunk).
struct WgJob {
  const float *dz, *x;
  float *slab, *bslab;
  int ldx;
};
struct WgJobs {
  WgJob job[4];
  int chunks, chunk_size;
};
constexpr int kWgSub = 32, kWgOt = 128, kWgPad = 4;
// One split-K tile of dW = DZ^T X: output rows [o0, o0 + 128) x k columns [k0, k0 + KT) of one job, summed over chunk
// `chunk` of csize samples (sa / sb: this block's double-buffered LDS staging, [2][32][128 + 4] and [2][32][KT + 4]).
template <int KT>
__device__ __forceinline__ void wgrad_tile(const WgJob &job, int bx, int by, int chunk, int csize,
                                           float (*sa)[kWgSub][kWgOt + kWgPad], float (*sb)[kWgSub][KT + kWgPad]) {
  constexpr int SUB = kWgSub, OT = kWgOt;
  constexpr int NB = KT == 128 ? 4 : 1;  // 16-column blocks per wave
  constexpr int LA = SUB * OT / 4 / WG, LB = (SUB * KT / 4 + WG - 1) / WG;  // f4 loads per thread per sub-chunk
  const float *__restrict__ dz = job.dz;
  const float *__restrict__ xs = job.x;
  float *__restrict__ slab = job.slab;
  float *__restrict__ bslab = job.bslab;
  const int ldx = job.ldx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kk = lane >> 4, i = lane & 15;
  const int wo = wave >> 1, wk = wave & 1;
  const int o0 = bx * OT, k0 = by * KT;
  const int64_t j0 = (int64_t)chunk * csize;
  const bool bias = bslab != nullptr && by == 0;
  f4 acc[4][NB];
#pragma unroll
  for (int bo = 0; bo < 4; ++bo)
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) acc[bo][bk] = z4();
  float bsum = 0.0f;  // thread t < OT: column o0 + t of DZ
  f4 ga[LA], gb[LB];
  auto fetch = [&](int sub) {
#pragma unroll
    for (int u = 0; u < LA; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (OT / 4), cc = (e % (OT / 4)) * 4;
      ga[u] = *reinterpret_cast<const f4 *>(dz + (j0 + sub + rr) * H + o0 + cc);
    }
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (KT / 4), cc = (e % (KT / 4)) * 4;
      if (e < SUB * KT / 4) gb[u] = *reinterpret_cast<const f4 *>(xs + (j0 + sub + rr) * ldx + k0 + cc);
    }
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int u = 0; u < LA; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (OT / 4), cc = (e % (OT / 4)) * 4;
      *reinterpret_cast<f4 *>(&sa[b][rr][cc]) = ga[u];
    }
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int e = threadIdx.x + u * WG, rr = e / (KT / 4), cc = (e % (KT / 4)) * 4;
      if (e < SUB * KT / 4) *reinterpret_cast<f4 *>(&sb[b][rr][cc]) = gb[u];
    }
  };
  fetch(0);
  for (int sub = 0, b = 0; sub < csize; sub += SUB, b ^= 1) {
    stash(b);
    __syncthreads();
    if (sub + SUB < csize) fetch(sub + SUB);
    if (bias && threadIdx.x < OT) {
      // the sub-chunk's 32 rows as four interleaved partial sums joined as a tree, then added to the chunk's sum:
      // one running sum over the chunk's 256 or 512 signed terms lost a few ulp more than torch's blocked column
      // sum does (tests/test_gpu_learner_kernels.py measures both against float64)
      float ps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < SUB; ++r) ps[r & 3] += sa[b][r][threadIdx.x];
      bsum += (ps[0] + ps[1]) + (ps[2] + ps[3]);
    }
#pragma unroll
    for (int s = 0; s < SUB / 4; ++s) {
      const f4 A = *reinterpret_cast<const f4 *>(&sa[b][4 * s + kk][64 * wo + 4 * i]);  // rows o = 64 wo + 4 i + bo
      f4 B;
      if constexpr (NB == 4) B = *reinterpret_cast<const f4 *>(&sb[b][4 * s + kk][64 * wk + 4 * i]);  // k = 64 wk + 4 i + bk
      else B[0] = sb[b][4 * s + kk][16 * wk + i];                                                // k = 16 wk + i
#pragma unroll
      for (int bo = 0; bo < 4; ++bo)
#pragma unroll
        for (int bk = 0; bk < NB; ++bk) acc[bo][bk] = mfma(A[bo], B[bk], acc[bo][bk]);
    }
  }
  if (bias && threadIdx.x < OT) bslab[(int64_t)chunk * H + o0 + threadIdx.x] = bsum;
  // acc[bo][bk] lane (jj = i, q = kk) reg r: o = o0 + 64 wo + 4 (4 q + r) + bo, k = k0 + (NB == 4 ? 64 wk + 4 jj + bk : 16 wk + jj)
  float *dst = slab + (int64_t)chunk * H * ldx;
#pragma unroll
  for (int bo = 0; bo < 4; ++bo)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = o0 + 64 * wo + 4 * (4 * kk + r) + bo;
      if constexpr (NB == 4) {
        const f4 v = f4{acc[bo][0][r], acc[bo][1][r], acc[bo][2][r], acc[bo][3][r]};
        *reinterpret_cast<f4 *>(dst + (int64_t)o * ldx + k0 + 64 * wk + 4 * i) = v;
      } else {
        dst[(int64_t)o * ldx + k0 + 16 * wk + i] = acc[bo][0][r];
      }
    }
}

template <int KT>
__global__ void __launch_bounds__(WG, 1) wgrad_kernel(WgJobs jobs) {
  __shared__ float sa[2][kWgSub][kWgOt + kWgPad];
  __shared__ float sb[2][kWgSub][KT + kWgPad];
  const int bz = blockIdx.z;
  wgrad_tile<KT>(jobs.job[bz / jobs.chunks], blockIdx.x, blockIdx.y, bz % jobs.chunks, jobs.chunk_size, sa, sb);
}

// hkl_wgrad_pair: a network's dW2 tiles (k width 256) and dW1 tiles (k width 32) in one launch -- blocks
// [0, n_wide) take the wide jobs (grid 2 x 2 x chunks per job), the rest the narrow ones (2 x 1 x chunks), so the
// short dW1 tiles fill the SIMDs the dW2 tiles leave and one launch gap is saved.  The narrow tile's staging
// lives inside the wide one's (same LDS as a wide-only block).
// One block of the pair: jobs are read through job_of(width, j), which the single kernel answers from its by-value
// WgJobs and the grouped one from member blockIdx.y's hkl_wgrad_job rows in device memory.
template <class JobOf>
__device__ __forceinline__ void wgrad_pair_body(const JobOf &job_of, int chunks_wide, int csize_wide, int chunks_narrow,
                                                int csize_narrow, int n_wide) {
  __shared__ float sa[2][kWgSub][kWgOt + kWgPad];
  __shared__ float sb[2][kWgSub][128 + kWgPad];
  static_assert(sizeof(float[2][kWgSub][XP + kWgPad]) <= sizeof(sb), "the narrow staging fits the wide one");
  const int id = blockIdx.x;
  if (id < n_wide) {
    const int z = id >> 2;
    wgrad_tile<128>(job_of(true, z / chunks_wide), id & 1, (id >> 1) & 1, z % chunks_wide, csize_wide, sa, sb);
  } else {
    const int j = id - n_wide, z = j >> 1;
    wgrad_tile<XP>(job_of(false, z / chunks_narrow), j & 1, 0, z % chunks_narrow, csize_narrow, sa,
                   reinterpret_cast<float(*)[kWgSub][XP + kWgPad]>(&sb[0][0][0]));
  }
}
__global__ void __launch_bounds__(WG, 1) wgrad_pair_kernel(WgJobs wide, WgJobs narrow, int n_wide) {
  wgrad_pair_body([&](bool w, int j) -> const WgJob & { return w ? wide.job[j] : narrow.job[j]; }, wide.chunks,
                  wide.chunk_size, narrow.chunks, narrow.chunk_size, n_wide);
}
// member blockIdx.y's jobs: rows [m * n_jobs, (m + 1) * n_jobs) of the two device arrays
struct WgGroup {
  const hkl_wgrad_job *wide, *narrow;
  int n_wide_jobs, n_narrow_jobs;
  int chunks_wide, csize_wide, chunks_narrow, csize_narrow;
  int n_wide;  // wide blocks per member
};
__global__ void __launch_bounds__(WG, 1) wgrad_pair_group_kernel(WgGroup g) {
  const int m = blockIdx.y;
  wgrad_pair_body(
      [&](bool w, int j) {
        const hkl_wgrad_job &d = w ? g.wide[m * g.n_wide_jobs + j] : g.narrow[m * g.n_narrow_jobs + j];
        return WgJob{d.dz, d.x, d.slab, d.bias_slab, w ? 256 : XP};
      },
      g.chunks_wide, g.csize_wide, g.chunks_narrow, g.csize_narrow, g.n_wide);
}

// ------------------------------------------------------------------------------------------------ Adam
// grad(e) = sum over chunks c (in order) of src[c * stride + row(e) * ld + col(e)]; then torch.optim.Adam (L2 weight
// decay, bias-corrected moments).  step: the optimiser's step count before this update (device, advanced by pack).
__device__ __forceinline__ void adam_body(const hkl_adam_io &io) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int sidx = -1;
  int64_t base = 0;
  for (int s = 0; s < io.n_seg; ++s) {
    const int64_t n = (int64_t)io.seg[s].rows * io.seg[s].cols;
    if (e < base + n) {
      sidx = s;
      break;
    }
    base += n;
  }
  if (sidx >= 0) {
    const hkl_seg &S = io.seg[sidx];
    const int64_t k = e - base;
    const int64_t rr = k / S.cols, cc = k % S.cols;
    const float *src = S.src + rr * S.ld + cc;
    // 16 partial sums (chunk c into p16[c & 15], in increasing c), summed in a fixed tree; up to 64 slab loads in
    // flight per thread (the reduction is bound by memory-level parallelism: ~2 workgroups per CU at the C5
    // parameter counts)
    float p16[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) p16[u] = 0.0f;
    int c = 0;
    for (; c + 64 <= S.chunks; c += 64) {  // four rounds' loads in flight at once, added in the same order
      float q[64];
#pragma unroll
      for (int u = 0; u < 64; ++u) q[u] = src[(int64_t)(c + u) * S.stride];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 16; ++u) p16[u] += q[16 * r + u];
    }
    for (; c + 32 <= S.chunks; c += 32) {  // two rounds' loads in flight at once, added in the same order
      float q[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) q[u] = src[(int64_t)(c + u) * S.stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) p16[u] += q[u];
#pragma unroll
      for (int u = 0; u < 16; ++u) p16[u] += q[16 + u];
    }
    for (; c + 16 <= S.chunks; c += 16) {
      float q[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) q[u] = src[(int64_t)(c + u) * S.stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) p16[u] += q[u];
    }
    for (; c < S.chunks; ++c) p16[c & 15] += src[(int64_t)c * S.stride];
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
      for (int u = 0; u < h; ++u) p16[u] = p16[u] + p16[u + h];
    float g = p16[0];
    float p = S.param[k];
    if (io.wd != 0.0f) g += io.wd * p;
    const float t = (float)(*io.step + 1);
    float m = S.m[k], v = S.v[k];
    // 1 - beta is taken in double and then rounded, as torch rounds its Python scalar: 1.0f - 0.999f is 1.3e-5 off
    // 0.001 (and 1.0f - 0.9f 2.4e-7 off 0.1), a scale error on every v (m) that no summation order accounts for
    const float beta1 = (float)io.beta1, beta2 = (float)io.beta2;
    const float omb1 = (float)(1.0 - io.beta1), omb2 = (float)(1.0 - io.beta2);
    m = m + (g - m) * omb1;  // exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + omb2 * g * g;
    const float bc1 = 1.0f - powf(beta1, t), bc2 = 1.0f - powf(beta2, t);
    const float denom = sqrtf(v) / sqrtf(bc2) + io.eps;
    p = p - (io.lr / bc1) * (m / denom);
    S.m[k] = m;
    S.v[k] = v;
    S.param[k] = p;
    if (io.polyak && S.target)  // soft_update with the new parameter: target.mul_(rho).add_(tau * param)
      S.target[k] = __fadd_rn(__fmul_rn(S.target[k], io.polyak_rho), __fmul_rn(io.polyak_tau, p));
  }
  if (blockIdx.x == 0 && io.loss_src) {
    // the step's loss: the sum of the workgroup partials (scaled), into the learner's accumulator -- a fixed-order
    // tree over workgroup 0's 256 threads (one thread summing 256 dependent loads was this kernel's tail)
    __shared__ float lred[256];
    float s = 0.0f;
    for (int c = threadIdx.x; c < io.loss_chunks; c += 256) s += io.loss_src[c];
    lred[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
      if ((int)threadIdx.x < h) lred[threadIdx.x] = lred[threadIdx.x] + lred[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      *io.loss_sum += (double)(lred[0] * io.loss_scale);
      *io.loss_count += 1.0;
    }
  }
}
__global__ void __launch_bounds__(256) adam_kernel(hkl_adam_io io) { adam_body(io); }
__global__ void __launch_bounds__(256) adam_group_kernel(const hkl_adam_io *__restrict__ ios) {
  adam_body(ios[blockIdx.y]);
}

// target <- target * rho + tau * param (learner.py:214-218: mul_(rho), add_((1 - rho) * param); tau = 1 - rho
// rounded to fp32 like the reference's scalar)
__global__ void __launch_bounds__(256) polyak_kernel(float *__restrict__ t, const float *__restrict__ p, int64_t n, float rho,
                                                     float tau) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) t[e] = t[e] * rho + tau * p[e];
}

__global__ void tanh_probe_kernel(const float *x, float *y, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) y[e] = tanh_fast(x[e]);
}

// ------------------------------------------------------------------------------------------------ packing
__device__ __forceinline__ void pack_body(const hkl_pack_io &io) {
  const hkl_net &N = io.net[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.y == 0 && e == 0 && io.step) *io.step += 1;  // the optimiser step this pack follows
  if (e >= kPackFloats) return;
  float *pk = N.pack;
  float v = 0.0f;
  if (e < kF1) {
    const int ob = (int)(e / 512), l = (int)(e / 8 % 64), s = (int)(e % 8);
    const int o = 16 * ob + (l & 15), c = 4 * s + (l >> 4);
    v = (s < S1 && c < N.n_in) ? N.w1[o * N.n_in + c] : 0.0f;
  } else if (e < kF1 + kFp) {
    const int64_t k = e - kF1;
    const int ob = (int)(k / 4096), kb = (int)(k / 256 % 16), l = (int)(k / 4 % 64), r = (int)(k % 4);
    v = N.w2[(16 * ob + (l & 15)) * H + 16 * kb + 4 * (l >> 4) + r];
  } else if (e < kF1 + kFp + kBp) {
    const int64_t k = e - kF1 - kFp;
    const int ib = (int)(k / 4096), ob = (int)(k / 256 % 16), l = (int)(k / 4 % 64), r = (int)(k % 4);
    v = N.w2[(16 * ob + 4 * (l >> 4) + r) * H + 16 * ib + (l & 15)];
  } else if (e < kF1 + kFp + kBp + kFo) {
    const int64_t k = e - kF1 - kFp - kBp;
    const int kb = (int)(k / 256), l = (int)(k / 4 % 64), r = (int)(k % 4);
    const int o = l & 15;
    v = o < N.n_out ? N.w3[o * H + 16 * kb + 4 * (l >> 4) + r] : 0.0f;
  } else {
    const int64_t k = e - kF1 - kFp - kBp - kFo;
    const int n = (int)(k / 4), c = (int)(k % 4);
    v = N.n_in == 22 ? N.w1[n * 22 + 18 + c] : 0.0f;
  }
  pk[e] = v;
}
__global__ void __launch_bounds__(256) pack_kernel(hkl_pack_io io) { pack_body(io); }
__global__ void __launch_bounds__(256) pack_group_kernel(const hkl_pack_io *__restrict__ ios) {
  pack_body(ios[blockIdx.z]);
}

}  // namespace hkl

using namespace hkl;

// ------------------------------------------------------------------------------------------------ C ABI
static thread_local char g_err[256];
static int fail(hipError_t e, const char *who) {
  snprintf(g_err, sizeof g_err, "%s: %s", who, hipGetErrorString(e));
  return HKL_E_DEVICE;
}

extern "C" {

const char *hkl_last_error(void) { return g_err; }

int hkl_pack(const hkl_net *nets, int n_nets, int64_t *step, void *stream) {
  if (n_nets < 1 || n_nets > 4) return HKL_E_INVALID;
  hkl_pack_io io{};
  for (int k = 0; k < n_nets; ++k) io.net[k] = nets[k];
  io.step = step;
  hipLaunchKernelGGL(pack_kernel, dim3((kPackFloats + 255) / 256, n_nets), dim3(256), 0, (hipStream_t)stream, io);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_pack");
}

int hkl_critic_step(const hkl_critic_io *io, void *stream) {
  if (!io || io->batch <= 0 || io->batch % CHUNK) return HKL_E_INVALID;
  hipLaunchKernelGGL(critic_step_kernel, dim3(io->batch / 64), dim3(WG), 0, (hipStream_t)stream, *io);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_critic_step");
}

int hkl_actor_step(const hkl_actor_io *io, void *stream) {
  if (!io || io->batch <= 0 || io->batch % CHUNK) return HKL_E_INVALID;
  hipLaunchKernelGGL(actor_step_kernel, dim3(io->batch / 64), dim3(WG), 0, (hipStream_t)stream, *io);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_actor_step");
}

// samples per split-K chunk (include/hockey_learner.h hkl_wgrad): a single k-width-256 job has 4 x B / 512 tiles
// at 512, half the workgroups the chip holds at C5's batch, so it takes 256-sample chunks
static int wg_chunk_size(int n_jobs, int k_width, int64_t batch) {
  return (k_width == 256 && n_jobs >= 2 && batch % 512 == 0) ? 512 : 256;
}

int hkl_wgrad(const hkl_wgrad_job *jobs, int n_jobs, int k_width, int64_t batch, void *stream) {
  if (!jobs || n_jobs < 1 || n_jobs > 4 || batch <= 0 || batch % CHUNK || (k_width != 256 && k_width != XP))
    return HKL_E_INVALID;
  WgJobs J{};
  for (int k = 0; k < n_jobs; ++k) J.job[k] = WgJob{jobs[k].dz, jobs[k].x, jobs[k].slab, jobs[k].bias_slab, k_width};
  // dW2 (k width 256): 512-sample chunks when the batch allows and two or more networks fill the chip (fewer
  // partial slabs for adam to add); one network (the actor) or dW1 (k width 32, a small tile per block): 256, for
  // more blocks
  J.chunk_size = wg_chunk_size(n_jobs, k_width, batch);
  J.chunks = (int)(batch / J.chunk_size);
  const unsigned z = (unsigned)(J.chunks * n_jobs);
  if (k_width == 256) hipLaunchKernelGGL(wgrad_kernel<128>, dim3(2, 2, z), dim3(WG), 0, (hipStream_t)stream, J);
  else hipLaunchKernelGGL(wgrad_kernel<32>, dim3(2, 1, z), dim3(WG), 0, (hipStream_t)stream, J);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_wgrad");
}

static WgJobs wg_jobs(const hkl_wgrad_job *jobs, int n_jobs, int k_width, int64_t batch) {
  WgJobs J{};
  for (int k = 0; k < n_jobs; ++k) J.job[k] = WgJob{jobs[k].dz, jobs[k].x, jobs[k].slab, jobs[k].bias_slab, k_width};
  J.chunk_size = wg_chunk_size(n_jobs, k_width, batch);
  J.chunks = (int)(batch / J.chunk_size);
  return J;
}

int hkl_wgrad_pair(const hkl_wgrad_job *wide, int n_wide, const hkl_wgrad_job *narrow, int n_narrow, int64_t batch,
                   void *stream) {
  if (!wide || !narrow || n_wide < 1 || n_wide > 4 || n_narrow < 1 || n_narrow > 4 || batch <= 0 || batch % CHUNK)
    return HKL_E_INVALID;
  const WgJobs W = wg_jobs(wide, n_wide, 256, batch), N = wg_jobs(narrow, n_narrow, XP, batch);
  const int nw = 4 * W.chunks * n_wide, nn = 2 * N.chunks * n_narrow;
  hipLaunchKernelGGL(wgrad_pair_kernel, dim3((unsigned)(nw + nn)), dim3(WG), 0, (hipStream_t)stream, W, N, nw);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_wgrad_pair");
}

int hkl_adam(const hkl_adam_io *io, void *stream) {
  if (!io || io->n_seg < 1 || io->n_seg > HKL_MAX_SEG) return HKL_E_INVALID;
  if (io->loss_src && (!io->loss_sum || !io->loss_count)) return HKL_E_INVALID;  // loss partials need a destination
  for (int s = 0; s < io->n_seg; ++s)
    if (!io->seg[s].param || !io->seg[s].m || !io->seg[s].v || !io->seg[s].src || (io->polyak && !io->seg[s].target))
      return HKL_E_INVALID;
  int64_t n = 0;
  for (int s = 0; s < io->n_seg; ++s) n += (int64_t)io->seg[s].rows * io->seg[s].cols;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *io);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_adam");
}

int hkl_polyak(float *target, const float *param, int64_t n, float rho, float tau, void *stream) {
  if (n <= 0) return HKL_E_INVALID;
  hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, target, param,
                     n, rho, tau);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_polyak");
}

int hkl_pack_floats(void) { return kPackFloats; }

int hkl_sample(const hkl_sample_io *io, void *stream) {
  if (!io || io->batch <= 0) return HKL_E_INVALID;
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((io->batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *io);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_sample");
}

// ---- grouped forms (include/hockey_learner.h): every member's struct is checked on the host copy, then one launch
// reads the device copy.  bad_*: what is wrong with one member's struct, or nullptr.
static bool null_net(const hkl_net &n) { return !n.w1 || !n.b1 || !n.w2 || !n.b2 || !n.w3 || !n.b3 || !n.pack; }
static const char *bad_batch(int64_t b) { return (b <= 0 || b % CHUNK) ? "batch is not a positive multiple of 256" : nullptr; }
static const char *bad_sample(const hkl_sample_io &io) {
  if (const char *w = bad_batch(io.batch)) return w;
  return (!io.counter || !io.size || !io.idx || !io.noise) ? "null counter / size / idx / noise" : nullptr;
}
static const char *bad_critic(const hkl_critic_io &io) {
  if (const char *w = bad_batch(io.batch)) return w;
  if (!io.idx || !io.ring_s || !io.ring_a || !io.ring_r || !io.ring_s2 || !io.ring_d || !io.noise)
    return "null idx / ring column / noise";
  if (null_net(io.target_actor) || null_net(io.target_q[0]) || null_net(io.target_q[1]) || null_net(io.q[0]) ||
      null_net(io.q[1]))
    return "null network pointer";
  if (!io.x0 || !io.p_loss) return "null x0 / p_loss";
  for (int k = 0; k < 2; ++k)
    if (!io.h1[k] || !io.dz1[k] || !io.dz2[k] || !io.p_dw3[k] || !io.p_db3[k]) return "null h1 / dz1 / dz2 / p_dw3 / p_db3";
  return nullptr;
}
static const char *bad_actor(const hkl_actor_io &io) {
  if (const char *w = bad_batch(io.batch)) return w;
  if (!io.idx || !io.ring_s) return "null idx / ring_s";
  if (null_net(io.actor) || null_net(io.q1)) return "null network pointer";
  if (!io.x0 || !io.h1 || !io.h2 || !io.dz1 || !io.dz2 || !io.p_dw3 || !io.p_db3 || !io.p_loss)
    return "null x0 / h1 / h2 / dz1 / dz2 / p_dw3 / p_db3 / p_loss";
  return nullptr;
}
static const char *bad_adam(const hkl_adam_io &io) {
  if (io.n_seg < 1 || io.n_seg > HKL_MAX_SEG) return "n_seg outside [1, HKL_MAX_SEG]";
  if (io.loss_src && (!io.loss_sum || !io.loss_count)) return "loss partials without loss_sum / loss_count";
  if (!io.step) return "null step";
  for (int s = 0; s < io.n_seg; ++s)
    if (!io.seg[s].param || !io.seg[s].m || !io.seg[s].v || !io.seg[s].src || (io.polyak && !io.seg[s].target))
      return "null segment pointer";
  return nullptr;
}
static int bad_group(const char *who, const void *host, const void *dev, int n_members) {
  if (n_members < 1 || n_members > HKL_GROUP_MAX)
    snprintf(g_err, sizeof g_err, "%s: n_members %d outside [1, %d]", who, n_members, HKL_GROUP_MAX);
  else if (!host || !dev) snprintf(g_err, sizeof g_err, "%s: null %s array", who, host ? "dev" : "host");
  else return 0;
  return HKL_E_INVALID;
}
static int bad_member(const char *who, int m, const char *what) {
  snprintf(g_err, sizeof g_err, "%s: member %d: %s", who, m, what);
  return HKL_E_INVALID;
}
static int launched(const char *who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, who);
}

int hkl_sample_group(const hkl_sample_io *host, const hkl_sample_io *dev, int n_members, void *stream) {
  const char *who = "hkl_sample_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_sample(host[m])) return bad_member(who, m, w);
    if (host[m].batch != host[0].batch) return bad_member(who, m, "batch differs from member 0's");
  }
  hipLaunchKernelGGL(sample_group_kernel, dim3((unsigned)(host[0].batch / 256), n_members), dim3(256), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_critic_step_group(const hkl_critic_io *host, const hkl_critic_io *dev, int n_members, void *stream) {
  const char *who = "hkl_critic_step_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_critic(host[m])) return bad_member(who, m, w);
    if (host[m].batch != host[0].batch) return bad_member(who, m, "batch differs from member 0's");
  }
  hipLaunchKernelGGL(critic_step_group_kernel, dim3((unsigned)(host[0].batch / 64), n_members), dim3(WG), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_actor_step_group(const hkl_actor_io *host, const hkl_actor_io *dev, int n_members, void *stream) {
  const char *who = "hkl_actor_step_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_actor(host[m])) return bad_member(who, m, w);
    if (host[m].batch != host[0].batch) return bad_member(who, m, "batch differs from member 0's");
  }
  hipLaunchKernelGGL(actor_step_group_kernel, dim3((unsigned)(host[0].batch / 64), n_members), dim3(WG), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_wgrad_pair_group(const hkl_wgrad_job *wide_host, const hkl_wgrad_job *wide_dev, int n_wide,
                         const hkl_wgrad_job *narrow_host, const hkl_wgrad_job *narrow_dev, int n_narrow, int64_t batch,
                         int n_members, void *stream) {
  const char *who = "hkl_wgrad_pair_group";
  if (bad_group(who, wide_host, wide_dev, n_members) || bad_group(who, narrow_host, narrow_dev, n_members))
    return HKL_E_INVALID;
  if (n_wide < 1 || n_wide > 4 || n_narrow < 1 || n_narrow > 4 || bad_batch(batch)) {
    snprintf(g_err, sizeof g_err, "%s: n_wide / n_narrow outside [1, 4], or the batch is not a positive multiple of 256", who);
    return HKL_E_INVALID;
  }
  for (int m = 0; m < n_members; ++m) {
    for (int k = 0; k < n_wide; ++k)
      if (const hkl_wgrad_job &j = wide_host[m * n_wide + k]; !j.dz || !j.x || !j.slab)
        return bad_member(who, m, "null dz / x / slab of a wide job");
    for (int k = 0; k < n_narrow; ++k)
      if (const hkl_wgrad_job &j = narrow_host[m * n_narrow + k]; !j.dz || !j.x || !j.slab)
        return bad_member(who, m, "null dz / x / slab of a narrow job");
  }
  WgGroup g{};
  g.wide = wide_dev;
  g.narrow = narrow_dev;
  g.n_wide_jobs = n_wide;
  g.n_narrow_jobs = n_narrow;
  g.csize_wide = wg_chunk_size(n_wide, 256, batch);  // the chunking of hkl_wgrad_pair at these job counts
  g.csize_narrow = wg_chunk_size(n_narrow, XP, batch);
  g.chunks_wide = (int)(batch / g.csize_wide);
  g.chunks_narrow = (int)(batch / g.csize_narrow);
  g.n_wide = 4 * g.chunks_wide * n_wide;
  const int nn = 2 * g.chunks_narrow * n_narrow;
  hipLaunchKernelGGL(wgrad_pair_group_kernel, dim3((unsigned)(g.n_wide + nn), n_members), dim3(WG), 0,
                     (hipStream_t)stream, g);
  return launched(who);
}

int hkl_adam_group(const hkl_adam_io *host, const hkl_adam_io *dev, int n_members, void *stream) {
  const char *who = "hkl_adam_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  int64_t n = 0;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_adam(host[m])) return bad_member(who, m, w);
    if (host[m].n_seg != host[0].n_seg) return bad_member(who, m, "n_seg differs from member 0's");
    for (int s = 0; s < host[m].n_seg; ++s)
      if (host[m].seg[s].rows != host[0].seg[s].rows || host[m].seg[s].cols != host[0].seg[s].cols)
        return bad_member(who, m, "a segment's rows x cols differ from member 0's");
  }
  for (int s = 0; s < host[0].n_seg; ++s) n += (int64_t)host[0].seg[s].rows * host[0].seg[s].cols;
  hipLaunchKernelGGL(adam_group_kernel, dim3((unsigned)((n + 255) / 256), n_members), dim3(256), 0, (hipStream_t)stream,
                     dev);
  return launched(who);
}

int hkl_pack_group(const hkl_pack_io *host, const hkl_pack_io *dev, int n_nets, int n_members, void *stream) {
  const char *who = "hkl_pack_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  if (n_nets < 1 || n_nets > 4) {
    snprintf(g_err, sizeof g_err, "%s: n_nets %d outside [1, 4]", who, n_nets);
    return HKL_E_INVALID;
  }
  for (int m = 0; m < n_members; ++m)
    for (int k = 0; k < n_nets; ++k)
      if (null_net(host[m].net[k])) return bad_member(who, m, "null network pointer");
  hipLaunchKernelGGL(pack_group_kernel, dim3((kPackFloats + 255) / 256, n_nets, n_members), dim3(256), 0,
                     (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_tanh_probe(const float *x, float *y, int64_t n, void *stream) {
  if (n <= 0) return HKL_E_INVALID;
  hipLaunchKernelGGL(tanh_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_tanh_probe");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ prioritized replay
// Prioritized replay (rl/replay/prioritized_buffer.py) on per-block sums; uses philox / sample_noise and fail above.
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

static bool per_ok(const hkl_per *p) {
  return p && p->cap > 0 && p->w && p->size && p->bsum && p->bmax && p->bpre && p->last && p->bown;
}
static int64_t per_nblk(const hkl_per *p) { return (p->cap + HKL_PER_BLOCK - 1) / HKL_PER_BLOCK; }
static void per_refresh_launch(const hkl_per *p, int64_t lo, int64_t n, int64_t size_arg, hipStream_t st) {
  const int64_t b0 = lo / HKL_PER_BLOCK, nb = (lo + n - 1) / HKL_PER_BLOCK - b0 + 1;
  hipLaunchKernelGGL(hkl::per_refresh_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, *p, b0, nb, size_arg);
}

extern "C" {

int hkl_per_block(void) { return HKL_PER_BLOCK; }

int hkl_per_refresh(const hkl_per *per, int64_t lo, int64_t n, void *stream) {
  if (!per_ok(per) || lo < 0 || n <= 0 || n > per->cap || lo > per->cap - n) return HKL_E_INVALID;
  per_refresh_launch(per, lo, n, -1, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_per_refresh");
}

int hkl_per_push(const hkl_per *per, int64_t pos, int64_t n, int64_t size_after, void *stream) {
  if (!per_ok(per) || pos < 0 || pos >= per->cap || n <= 0 || n > per->cap || size_after < n || size_after > per->cap)
    return HKL_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(hkl::per_push_kernel, dim3(1), dim3(1024), 0, st, *per, pos, n, size_after);
  const int64_t head = per->cap - pos < n ? per->cap - pos : n;
  per_refresh_launch(per, pos, head, size_after, st);
  if (head < n) per_refresh_launch(per, 0, n - head, size_after, st);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_per_push");
}

static bool per_iw_ok(const hkl_per_sample_io *io) {
  return io && per_ok(&io->per) && io->batch > 0 && io->batch < ((int64_t)1 << 31) && io->idx;
}

int hkl_per_weights(const hkl_per_sample_io *io, void *stream) {
  if (!per_iw_ok(io) || !io->iw) return HKL_E_INVALID;
  hipLaunchKernelGGL(hkl::per_iw_kernel, dim3((unsigned)((io->batch + 1023) / 1024)), dim3(1024), 0,
                     (hipStream_t)stream, io->per, io->idx, io->iw, io->batch, io->beta);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_per_weights");
}

int hkl_per_sample(const hkl_per_sample_io *io, void *stream) {
  if (!per_iw_ok(io) || (!io->u && !io->counter)) return HKL_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = per_nblk(&io->per);
  hipLaunchKernelGGL(hkl::per_prefix_kernel, dim3(1), dim3(1024), 0, st, io->per, nblk);
  hipLaunchKernelGGL(hkl::per_sample_kernel, dim3((unsigned)((io->batch + 3) / 4)), dim3(256), 0, st, *io, nblk);
  if (io->iw)
    hipLaunchKernelGGL(hkl::per_iw_kernel, dim3((unsigned)((io->batch + 1023) / 1024)), dim3(1024), 0, st, io->per,
                       io->idx, io->iw, io->batch, io->beta);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_per_sample");
}

int hkl_per_update(const hkl_per_update_io *io, void *stream) {
  if (!io || !per_ok(&io->per) || io->batch <= 0 || io->batch >= ((int64_t)1 << 31) || !io->idx || !io->td)
    return HKL_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned g = (unsigned)((io->batch + 255) / 256);
  hipLaunchKernelGGL(hkl::per_mark_kernel, dim3(g), dim3(256), 0, st, *io);
  hipLaunchKernelGGL(hkl::per_write_kernel, dim3(g), dim3(256), 0, st, *io);
  hipLaunchKernelGGL(hkl::per_touch_kernel, dim3((unsigned)((io->batch + 3) / 4)), dim3(256), 0, st, *io);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_per_update");
}

// ---- grouped forms (include/hockey_learner.h): the single calls' checks on every member of the host copy, then the
// single calls' launches with the member in blockIdx.y.  bad_per*: what is wrong with one member, or nullptr.
static const char *bad_per(const hkl_per &p) {
  if (p.cap <= 0) return "cap is not positive";
  if (!p.w || !p.size || !p.bsum || !p.bmax || !p.bpre || !p.last || !p.bown)
    return "null w / size / bsum / bmax / bpre / last / bown";
  // per_load reads a lane's sub-chunk as four float4: the single ring's allocation is aligned, a slice of a shared
  // storage has to be placed so
  return ((uintptr_t)p.w % 16) ? "w is not 16-byte aligned" : nullptr;
}
static const char *bad_per_iw(const hkl_per_sample_io &io) {
  if (const char *w = bad_per(io.per)) return w;
  if (io.batch <= 0 || io.batch >= ((int64_t)1 << 31)) return "batch outside [1, 2^31)";
  return io.idx ? nullptr : "null idx";
}
static const char *bad_per_update(const hkl_per_update_io &io) {
  if (const char *w = bad_per(io.per)) return w;
  if (io.batch <= 0 || io.batch >= ((int64_t)1 << 31)) return "batch outside [1, 2^31)";
  return (io.idx && io.td) ? nullptr : "null idx / td";
}
// the members' grids agree: one cap (so one block count) and one batch
#define HKL_PER_SAME(field, what) \
  if (host[m].field != host[0].field) return bad_member(who, m, what " differs from member 0's")

int hkl_per_refresh_group(const hkl_per *host, const hkl_per *dev, int n_members, void *stream) {
  const char *who = "hkl_per_refresh_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_per(host[m])) return bad_member(who, m, w);
    HKL_PER_SAME(cap, "cap");
  }
  const int64_t nblk = per_nblk(&host[0]);
  hipLaunchKernelGGL(hkl::per_refresh_group_kernel, dim3((unsigned)((nblk + 3) / 4), n_members), dim3(256), 0,
                     (hipStream_t)stream, dev, nblk);
  return launched(who);
}

int hkl_per_push_group(const hkl_per *host, const hkl_per *dev, const int64_t *pos, const int64_t *n,
                       const int64_t *size_after, int64_t max_n, int n_members, void *stream) {
  const char *who = "hkl_per_push_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_per(host[m])) return bad_member(who, m, w);
    HKL_PER_SAME(cap, "cap");
  }
  if (!pos || !n || !size_after) {
    snprintf(g_err, sizeof g_err, "%s: null pos / n / size_after array", who);
    return HKL_E_INVALID;
  }
  if (max_n < 1 || max_n > host[0].cap) {
    snprintf(g_err, sizeof g_err, "%s: max_n %lld outside [1, cap = %lld]", who, (long long)max_n,
             (long long)host[0].cap);
    return HKL_E_INVALID;
  }
  const hipStream_t st = (hipStream_t)stream;
  // the blocks a push of max_n slots can cover: a head that starts anywhere in a block, a tail that starts at slot 0
  const int64_t nblk = per_nblk(&host[0]);
  int64_t n_head = (max_n + HKL_PER_BLOCK - 2) / HKL_PER_BLOCK + 1, n_tail = (max_n - 1 + HKL_PER_BLOCK - 1) / HKL_PER_BLOCK;
  n_head = n_head < nblk ? n_head : nblk;
  n_tail = n_tail < nblk ? n_tail : nblk;
  hipLaunchKernelGGL(hkl::per_push_group_kernel, dim3(1, n_members), dim3(1024), 0, st, dev, pos, n, size_after, max_n);
  hipLaunchKernelGGL(hkl::per_push_refresh_group_kernel, dim3((unsigned)((n_head + n_tail + 3) / 4), n_members),
                     dim3(256), 0, st, dev, pos, n, size_after, max_n, n_head, n_tail);
  return launched(who);
}

int hkl_per_weights_group(const hkl_per_sample_io *host, const hkl_per_sample_io *dev, int n_members, void *stream) {
  const char *who = "hkl_per_weights_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_per_iw(host[m])) return bad_member(who, m, w);
    if (!host[m].iw) return bad_member(who, m, "null iw");
    HKL_PER_SAME(per.cap, "cap");
    HKL_PER_SAME(batch, "batch");
  }
  hipLaunchKernelGGL(hkl::per_iw_group_kernel, dim3((unsigned)((host[0].batch + 1023) / 1024), n_members), dim3(1024),
                     0, (hipStream_t)stream, dev);
  return launched(who);
}

int hkl_per_sample_group(const hkl_per_sample_io *host, const hkl_per_sample_io *dev, int n_members, void *stream) {
  const char *who = "hkl_per_sample_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_per_iw(host[m])) return bad_member(who, m, w);
    if (!host[m].u && !host[m].counter) return bad_member(who, m, "null u and null counter");
    HKL_PER_SAME(per.cap, "cap");
    HKL_PER_SAME(batch, "batch");
  }
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = per_nblk(&host[0].per), batch = host[0].batch;
  hipLaunchKernelGGL(hkl::per_prefix_group_kernel, dim3(1, n_members), dim3(1024), 0, st, dev, nblk);
  hipLaunchKernelGGL(hkl::per_sample_group_kernel, dim3((unsigned)((batch + 3) / 4), n_members), dim3(256), 0, st, dev,
                     nblk);
  // always launched, so that the launch count does not depend on the members: one without iw leaves at once
  hipLaunchKernelGGL(hkl::per_iw_group_kernel, dim3((unsigned)((batch + 1023) / 1024), n_members), dim3(1024), 0, st,
                     dev);
  return launched(who);
}

int hkl_per_update_group(const hkl_per_update_io *host, const hkl_per_update_io *dev, int n_members, void *stream) {
  const char *who = "hkl_per_update_group";
  if (bad_group(who, host, dev, n_members)) return HKL_E_INVALID;
  for (int m = 0; m < n_members; ++m) {
    if (const char *w = bad_per_update(host[m])) return bad_member(who, m, w);
    HKL_PER_SAME(per.cap, "cap");
    HKL_PER_SAME(batch, "batch");
  }
  const hipStream_t st = (hipStream_t)stream;
  const int64_t batch = host[0].batch;
  const dim3 g((unsigned)((batch + 255) / 256), n_members);
  hipLaunchKernelGGL(hkl::per_mark_group_kernel, g, dim3(256), 0, st, dev);
  hipLaunchKernelGGL(hkl::per_write_group_kernel, g, dim3(256), 0, st, dev);
  hipLaunchKernelGGL(hkl::per_touch_group_kernel, dim3((unsigned)((batch + 3) / 4), n_members), dim3(256), 0, st, dev);
  return launched(who);
}
#undef HKL_PER_SAME

}  // extern "C"

// ------------------------------------------------------------------------------------------------ actor inference
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
template <class IO>
__device__ __forceinline__ void act_tile(const IO &io, int k, int start, int cnt, f4 *sfrag) {
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
  if (live) io.out[row * io.out_ld + io.out_col + q] = a;
}

__global__ void __launch_bounds__(WG, 1) act_kernel(hkl_act_io io) {
  __shared__ f4 sfrag[2 * 16 * 64 + 64];  // two fragment buffers + the staged bias
  // this workgroup's policy k and its rows [start, start + cnt) of the group, 64 per workgroup.  Everything up to
  // the return depends on blockIdx and the arguments alone, so a surplus workgroup leaves as a whole before the
  // first barrier.
  int k = 0, start = 0, cnt = 0;
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
    if (k == io.n_policies) return;
  } else {
    start = 64 * (int)blockIdx.x;
    cnt = io.n_rows - start;
  }
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

extern "C" {

int hkl_act_io_size(void) { return (int)sizeof(hkl_act_io); }
int hkl_act_wide_io_size(void) { return (int)sizeof(hkl_act_wide_io); }

int hkl_act_wide(const hkl_act_wide_io *io, void *stream) {
  if (!io || io->n_policies < 1 || io->n_policies > HKL_ACT_WIDE_MAX_POLICIES || io->n_rows < 0 || io->obs_ld < 18 ||
      io->out_col < 0 || io->out_ld < (int64_t)io->out_col + 4)
    return HKL_E_INVALID;
  if (!io->params || !io->packs || !io->obs || !io->out) return HKL_E_INVALID;
  if (io->policy && (!io->order || !io->counts || !io->offsets || !io->tiles)) return HKL_E_INVALID;
  if (io->n_rows == 0) return HKL_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = (io->n_rows + 63) / 64;
  if (io->policy) {
    const unsigned blocks = (unsigned)((io->n_rows + 255) / 256);
    hipLaunchKernelGGL(act_wide_zero_kernel, dim3((unsigned)(io->n_policies / 256 + 1)), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_wide_hist_kernel, dim3(blocks), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_wide_scan_kernel, dim3(1), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_wide_scatter_kernel, dim3(blocks), dim3(256), 0, st, *io);
    // the non-empty tiles are at most min(n_rows, n_rows / 64 + K); their number is known only on the device
    const int64_t bound = tiles + io->n_policies < io->n_rows ? tiles + io->n_policies : (int64_t)io->n_rows;
    hipLaunchKernelGGL(act_wide_kernel, dim3((unsigned)bound), dim3(WG), 0, st, *io);
  } else {
    hipLaunchKernelGGL(act_wide_kernel, dim3((unsigned)tiles), dim3(WG), 0, st, *io);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_act_wide");
}

int hkl_act(const hkl_act_io *io, void *stream) {
  if (!io || io->n_policies < 1 || io->n_policies > HKL_ACT_MAX_POLICIES || io->n_rows < 0 || io->obs_ld < 18 ||
      io->out_col < 0 || io->out_ld < (int64_t)io->out_col + 4)
    return HKL_E_INVALID;
  if (!io->params || !io->packs || !io->obs || !io->out) return HKL_E_INVALID;
  if (io->policy && (!io->order || !io->counts || !io->offsets)) return HKL_E_INVALID;
  if (io->n_rows == 0) return HKL_OK;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((io->n_rows + 63) / 64);
  if (io->policy) {
    const unsigned blocks = (unsigned)((io->n_rows + 255) / 256);
    const hipError_t m = hipMemsetAsync(io->counts, 0, sizeof(int32_t) * (HKL_ACT_MAX_POLICIES + 1), st);
    if (m != hipSuccess) return fail(m, "hkl_act");
    hipLaunchKernelGGL(act_hist_kernel, dim3(blocks), dim3(256), 0, st, *io);
    hipLaunchKernelGGL(act_scan_kernel, dim3(1), dim3(64), 0, st, *io);
    hipLaunchKernelGGL(act_scatter_kernel, dim3(blocks), dim3(256), 0, st, *io);
    // sum_k ceil(count_k / 64) <= n_rows / 64 + K tiles, known only on the device: the surplus workgroups return
    hipLaunchKernelGGL(act_kernel, dim3(tiles + (unsigned)io->n_policies), dim3(WG), 0, st, *io);
  } else {
    hipLaunchKernelGGL(act_kernel, dim3(tiles), dim3(WG), 0, st, *io);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, "hkl_act");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ twin-critic inference
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

static int invalid(const char *who, const char *what) {
  snprintf(g_err, sizeof g_err, "%s: %s", who, what);
  return HKL_E_INVALID;
}
static bool net_ok(const hkl_net &n) { return n.w1 && n.b1 && n.w2 && n.b2 && n.w3 && n.b3 && n.pack; }

extern "C" {

int hkl_value_io_size(void) { return (int)sizeof(hkl_value_io); }

int hkl_value(const hkl_value_io *io, void *stream) {
  const char *who = "hkl_value";
  if (!io) return invalid(who, "null io");
  if (io->n_rows < 0) return invalid(who, "n_rows < 0");
  if (!io->obs) return invalid(who, "null obs");
  if (io->obs_ld < 18) return invalid(who, "obs_ld < 18");
  if (io->act && io->act_ld < 4) return invalid(who, "act_ld < 4");
  if (io->act && io->act_out) return invalid(who, "act_out is the actor's action: not with act given");
  if (io->act_out && io->act_out_ld < 4) return invalid(who, "act_out_ld < 4");
  if (!io->q1 && !io->q2 && !io->qmin && !io->act_out) return invalid(who, "every output is null");
  if (!net_ok(io->q[0]) || !net_ok(io->q[1])) return invalid(who, "a critic's weight or pack pointer is null");
  if (!io->act && !net_ok(io->actor)) return invalid(who, "the actor's weight or pack pointer is null (act == NULL)");
  if (io->n_rows == 0) return HKL_OK;
  const unsigned tiles = (unsigned)(((int64_t)io->n_rows + 63) / 64);
  hipLaunchKernelGGL(value_kernel, dim3(tiles), dim3(WG), 0, (hipStream_t)stream, *io);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HKL_OK : fail(e, who);
}

}  // extern "C"
