// hkl_mlp.h -- the MFMA layer primitives every kernel of the learner library (hk_learner.hip) is built from.
// Every product is v_mfma_f32_16x16x4_f32: exact f32 fma chains (no reduced-precision path on gfx950), so the
// arithmetic is the reference's fp32 up to summation order.  Layout of a wave's activations ("Tile"): lane l holds
// sample j = l & 15 and, for each 16-neuron block ob and r = 0..3, neuron 16 ob + 4 (l >> 4) + r in v[ob][r] --
// exactly the C/D layout of the MFMA (col = lane & 15, row = 4 (lane >> 4) + reg), and, read as a B operand with
// k-step (kb, r), exactly the fragment the next layer needs (lane (j, kk = l >> 4) holds input neuron
// 16 kb + 4 kk + r).  Consecutive layers therefore chain in registers with no data movement; the weights are
// pre-packed into the matching A-operand order (pack_kernel) after every optimiser step.
#pragma once
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

}  // namespace hkl
