// Test-time tuning of the fused shape latent (OccBBoxHead.online_tuning, occ/latent_tune.py): what is specific to tuning
// around the decoder's backward chain.  The decoder is frozen, only the latent of every RoI moves, so
//   A  tune_head_lnbwd_kernel   loss gradient + head + LayerNorm/GELU backward of the last layer in one launch: the
//                               [M, 1024] gradient of y2 lives in registers only, no parameter-gradient partials
//   B  segment_sum_bf16_kernel  the gradient of the rows of a RoI summed into the RoI's row (f32, fixed order)
//   C  latent_ln_adam_kernel    LayerNorm backward of the latent and torch's Adam update in one pass over the row
// Row arithmetic of A: ln_math.hpp (the same formulas as ln_act_bwd_wide_kernel<2>, whose tiling this is).
#include <math.h>

#include "common.hpp"
#include "ln_math.hpp"

namespace {

constexpr int kHeadC = 1024;  // channels of the decoder's last hidden layer (kernel A)
constexpr int kSegC = 512;    // channels of its first hidden layer (kernel B)
// kernel A keeps gamma / beta / the head weights of a lane's 16 channels in registers (106 VGPRs: 4 waves per SIMD, 1024
// workgroups of 4 waves resident on 256 CUs): at most two rounds of workgroups, the rest of the rows grid-strided
constexpr int kTuneMaxBlocks = 2048;

__device__ __forceinline__ float wave_sum(float v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// A.  One wave per row, two 16-byte pieces per lane interleaved by 64 pieces (every load of a wave is one contiguous 1 KB).
__global__ void __launch_bounds__(256)
tune_head_lnbwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                       const float* __restrict__ weights, float scale, const float* __restrict__ head_w,
                       const uint16_t* __restrict__ z, const float* __restrict__ mean_rstd,
                       const float* __restrict__ gamma, const float* __restrict__ beta, int64_t n,
                       uint16_t* __restrict__ dz) {
  constexpr int VEC = 2, C = kHeadC;
  const int li = threadIdx.x & 63, rloc = threadIdx.x >> 6;
  ln_f32x2 g[VEC][4], b[VEC][4], hw[VEC][4];
#pragma unroll
  for (int u = 0; u < VEC; ++u) {
    const int ch = (u * 64 + li) * 8;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      g[u][p] = ln_f32x2{gamma[ch + 2 * p], gamma[ch + 2 * p + 1]};
      b[u][p] = ln_f32x2{beta[ch + 2 * p], beta[ch + 2 * p + 1]};
      hw[u][p] = ln_f32x2{head_w[ch + 2 * p], head_w[ch + 2 * p + 1]};
    }
  }
  for (int64_t r = (int64_t)blockIdx.x * 4 + rloc; r < n; r += (int64_t)gridDim.x * 4) {
    u32x4 xin[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) xin[u] = *(const u32x4*)(z + r * C + (u * 64 + li) * 8);
    const float mean = mean_rstd[r * 2], rstd = mean_rstd[r * 2 + 1];
    // d BCE-with-logits / d logit = sigmoid(logit) - label; exp overflows to inf for logit < -88: 1 / inf = 0, no NaN
    const float prob = 1.f / (1.f + __expf(-logits[r]));
    float d = scale * (prob - (float)labels[r]);
    if (weights) d *= weights[r];
    ln_f32x2 xh[VEC][4], dzg[VEC][4];
    ln_f32x2 a1 = {0.f, 0.f}, a2 = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      ln_unpack8(xin[u], xh[u]);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        xh[u][p] = (xh[u][p] - mean) * rstd;
        const ln_f32x2 dy = hw[u][p] * d;  // gradient of y2: never stored
        dzg[u][p] = (dy * ln_gelu_grad2(xh[u][p] * g[u][p] + b[u][p])) * g[u][p];
        a1 += dzg[u][p];
        a2 += dzg[u][p] * xh[u][p];
      }
    }
    const float s1 = wave_sum(a1.x + a1.y) * (1.f / C);
    const float s2 = wave_sum(a2.x + a2.y) * (1.f / C);
#pragma unroll
    for (int u = 0; u < VEC; ++u)
      *(u32x4*)(dz + r * C + (u * 64 + li) * 8) = ln_bwd_finish8(xh[u], dzg[u], rstd, s1, s2);
  }
}

// first row whose index is >= key (rows when there is none); any input leaves the result in [0, rows]
__device__ __forceinline__ int64_t lower_row(const int32_t* __restrict__ index, int64_t rows, int64_t key) {
  int64_t lo = 0, hi = rows;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)index[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// B.  Workgroup (k, s): segment k, the 64 channels of slice s.  8 lanes take the slice of one row (128 contiguous bytes),
// 32 rows are in flight per trip; the 32 row lanes are summed by shuffles inside each wave, then the 4 waves through LDS in
// a fixed order: the order of the additions depends on the segment's extent alone.
__global__ void __launch_bounds__(256)
segment_sum_bf16_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ index, int64_t rows,
                        float* __restrict__ out) {
  constexpr int C = kSegC;
  __shared__ int64_t range[2];
  __shared__ float part[4][64];
  const int64_t k = blockIdx.x;
  if (threadIdx.x < 2) range[threadIdx.x] = lower_row(index, rows, k + threadIdx.x);
  __syncthreads();
  const int64_t begin = range[0], end = range[1];
  const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int col = blockIdx.y * 64 + cl * 8;
  ln_f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  for (int64_t r = begin + rl; r < end; r += 32) {
    ln_f32x2 v[4];
    ln_unpack8(*(const u32x4*)(x + r * C + col), v);
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] += v[p];
  }
  float s[8] = {acc[0].x, acc[0].y, acc[1].x, acc[1].y, acc[2].x, acc[2].y, acc[3].x, acc[3].y};
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float t = s[j];
    t += __shfl_xor(t, 8, 64);
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (lane < 8) part[wave][lane * 8 + j] = t;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int t = threadIdx.x;
    out[k * C + blockIdx.y * 64 + t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
  }
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // the previous sum's readers are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// host numbers of one Adam step, worked out in double and rounded once (1 - 0.999f in f32 is 4.7e-5 off 0.001)
struct AdamStep {
  float beta2, one_minus_beta1, one_minus_beta2, eps;
  float step;      // lr_t / (1 - beta1^t)
  float sqrt_bc2;  // sqrt(1 - beta2^t)
};

// C.  One workgroup per latent row, up to two float4 pieces per thread (D <= 2048, D % 4 == 0).
__global__ void __launch_bounds__(256)
latent_ln_adam_kernel(float* __restrict__ e, const float* __restrict__ dn, float* __restrict__ m, float* __restrict__ v,
                      int32_t D, const float* __restrict__ gamma, float ln_eps, int use_ln, AdamStep a,
                      float* __restrict__ de_out) {
  __shared__ float red[4];
  const int64_t base = (int64_t)blockIdx.x * D;
  f32x4 x[2], gr[2];
  bool on[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ch = (threadIdx.x + j * 256) * 4;
    on[j] = ch < D;
    x[j] = on[j] ? *(const f32x4*)(e + base + ch) : f32x4{0.f, 0.f, 0.f, 0.f};
    gr[j] = on[j] ? *(const f32x4*)(dn + base + ch) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (use_ln) {
    const float inv_d = 1.f / (float)D;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) s += (x[j].x + x[j].y) + (x[j].z + x[j].w);
    const float mean = block_sum(s, red) * inv_d;
    f32x4 xh[2];
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      xh[j] = on[j] ? x[j] - mean : f32x4{0.f, 0.f, 0.f, 0.f};
      sq += (xh[j].x * xh[j].x + xh[j].y * xh[j].y) + (xh[j].z * xh[j].z + xh[j].w * xh[j].w);
    }
    const float rstd = 1.f / sqrtf(block_sum(sq, red) * inv_d + ln_eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (on[j]) {
        const int ch = (threadIdx.x + j * 256) * 4;
        xh[j] = xh[j] * rstd;
        gr[j] = gr[j] * *(const f32x4*)(gamma + ch);
      }
      s1 += (gr[j].x + gr[j].y) + (gr[j].z + gr[j].w);
      s2 += (gr[j].x * xh[j].x + gr[j].y * xh[j].y) + (gr[j].z * xh[j].z + gr[j].w * xh[j].w);
    }
    s1 = block_sum(s1, red) * inv_d;
    s2 = block_sum(s2, red) * inv_d;
#pragma unroll
    for (int j = 0; j < 2; ++j) gr[j] = ((gr[j] - s1) - xh[j] * s2) * rstd;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!on[j]) continue;
    const int ch = (threadIdx.x + j * 256) * 4;
    if (de_out) *(f32x4*)(de_out + base + ch) = gr[j];
    const f32x4 m0 = *(const f32x4*)(m + base + ch), v0 = *(const f32x4*)(v + base + ch);
    // torch.optim.Adam (single tensor): exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2);
    // denom = sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps; param.addcdiv_(exp_avg, denom, -lr / (1 - beta1^t))
    const f32x4 m1 = m0 + (gr[j] - m0) * a.one_minus_beta1;
    const f32x4 v1 = v0 * a.beta2 + (gr[j] * gr[j]) * a.one_minus_beta2;
    f32x4 p = x[j];
    p.x -= a.step * (m1.x / (sqrtf(v1.x) / a.sqrt_bc2 + a.eps));
    p.y -= a.step * (m1.y / (sqrtf(v1.y) / a.sqrt_bc2 + a.eps));
    p.z -= a.step * (m1.z / (sqrtf(v1.z) / a.sqrt_bc2 + a.eps));
    p.w -= a.step * (m1.w / (sqrtf(v1.w) / a.sqrt_bc2 + a.eps));
    *(f32x4*)(m + base + ch) = m1;
    *(f32x4*)(v + base + ch) = v1;
    *(f32x4*)(e + base + ch) = p;
  }
}

}  // namespace

extern "C" int ococc_occ_tune_head_lnbwd_bf16(const float* logits, const int32_t* labels, const float* weights,
                                              float scale, const float* head_weight, const uint16_t* z,
                                              const float* mean_rstd, const float* gamma, const float* beta,
                                              int64_t rows, int32_t c, uint16_t* dz, ococc_stream_t stream_) {
  OCOCC_REQUIRE(rows >= 0, "bad sizes");
  OCOCC_REQUIRE(c == kHeadC, "the decoder's last hidden layer has 1024 channels");
  if (rows == 0) return OCOCC_OK;
  OCOCC_REQUIRE(logits && labels && head_weight && z && mean_rstd && gamma && beta && dz, "null pointer");
  const int64_t blocks = ococc_cdiv(rows, 4);
  const int grid = (int)(blocks < kTuneMaxBlocks ? blocks : kTuneMaxBlocks);
  hipLaunchKernelGGL(tune_head_lnbwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream_, logits, labels, weights,
                     scale, head_weight, z, mean_rstd, gamma, beta, rows, dz);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_segment_sum_bf16(const uint16_t* x, const int32_t* index, int64_t rows, int32_t c, float* out,
                                      int64_t num_segments, ococc_stream_t stream_) {
  OCOCC_REQUIRE(rows >= 0 && num_segments >= 0 && num_segments <= 0x7fffffff, "bad sizes");
  OCOCC_REQUIRE(c == kSegC, "the decoder's first hidden layer has 512 channels");
  if (num_segments == 0) return OCOCC_OK;
  OCOCC_REQUIRE(out, "null pointer");
  if (rows == 0) {
    OCOCC_HIP(hipMemsetAsync(out, 0, (size_t)num_segments * kSegC * sizeof(float), (hipStream_t)stream_));
    return OCOCC_OK;
  }
  OCOCC_REQUIRE(x && index, "null pointer");
  hipLaunchKernelGGL(segment_sum_bf16_kernel, dim3((unsigned)num_segments, kSegC / 64), dim3(256), 0,
                     (hipStream_t)stream_, x, index, rows, out);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}

extern "C" int ococc_latent_ln_adam_f32(float* e, const float* d_n, float* m, float* v, int64_t rows, int32_t d,
                                        const float* gamma, float ln_eps, int32_t use_ln, double lr, double beta1,
                                        double beta2, double eps, int32_t t, float* de_out, ococc_stream_t stream_) {
  OCOCC_REQUIRE(rows >= 0 && rows <= 0x7fffffff, "bad sizes");
  OCOCC_REQUIRE(d >= 4 && d <= 2048 && d % 4 == 0, "D must be a multiple of 4 in [4, 2048]");
  OCOCC_REQUIRE(t >= 1, "t counts Adam steps from 1");
  OCOCC_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "betas must be in [0, 1)");
  if (rows == 0) return OCOCC_OK;
  OCOCC_REQUIRE(e && d_n && m && v && (!use_ln || gamma), "null pointer");
  AdamStep a;
  a.beta2 = (float)beta2;
  a.one_minus_beta1 = (float)(1.0 - beta1);
  a.one_minus_beta2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.step = (float)(lr / (1.0 - pow(beta1, (double)t)));
  a.sqrt_bc2 = (float)sqrt(1.0 - pow(beta2, (double)t));
  hipLaunchKernelGGL(latent_ln_adam_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream_, e, d_n, m, v, d,
                     gamma, ln_eps, use_ln ? 1 : 0, a, de_out);
  OCOCC_CHECK_LAUNCH();
  return OCOCC_OK;
}
