// layerwise.h -- layer-by-layer path for policies the fused kernel cannot hold on chip
// (hidden sizes > 64, obs dim > 31, any number of hidden layers incl. none).
//
// Same math as fused_policy.h, organised as fp32-MFMA GEMMs with fused epilogues over
// activations that stay resident in HBM for the whole update:
//   forward   H_{l+1} = tanh(H_l W_l^T + b_l)                        (NT GEMM + epilogue)
//   tangent   T_{l+1} = (H_l V_l^T + T_l W_l^T + c_l) (1 - H_{l+1}^2) (two NT GEMMs, one acc)
//   backward  D_l     = (D_{l+1} W_l) (1 - H_l^2)                     (NN GEMM + epilogue)
//   wgrad     gW_l    = D_{l+1}^T H_l                                  (TN GEMM, split over samples)
// Forward activations are cached per (batch, policy) binding, so the 10-25 Fisher-vector
// products of one CG solve reuse them (theta is fixed during CG).
//
// Reference semantics: mjrl/utils/fc_network.py:39-52, mjrl/policies/gaussian_mlp.py:99-145,
// mjrl/algos/batch_reinforce.py:40-58, mjrl/algos/npg_cg.py:62-81.
//
// Who owns what: lw_plan.h decides (switches, routes, split counts, GemmArgs builders; plain C++), lw_gemm.h / lw_gemm_p.h /
// lw_head.h hold the GEMM and output-layer kernels, lw_launch.h turns plans into launches, and this file keeps the small kernels
// and LayerwiseWS: the buffers, their validity, and the operations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "mfma_prims.h"
#include "launch_state.h"
#include "lw_head.h"
#include "lw_launch.h"
#include "vecops.h"

namespace mjx {

// x~ = (x - in_shift) / (in_scale + 1e-8)    fc_network.py:46
__global__ void k_normalize(const float* __restrict__ x, int64_t N, int n, int ldo, const float* __restrict__ tr, float* __restrict__ o) {
  // rows of o are padded to ldo = n rounded up to 4 floats (zeros): 16-byte operand granules for any observation width
  const int64_t tot = N * ldo;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i % ldo);
    const int64_t r = i / ldo;
    o[i] = (f < n) ? (x[r * n + f] - tr[f]) / (tr[n + f] + 1e-8f) : 0.f;
  }
}

// rows of `cols` floats <-> rows padded to `ld` floats (zeros): the first layer's weight block for observation widths
// that are not a multiple of 4 (the 39 / 45 / 46-wide Adroit observations)
__global__ void k_pad_rows(const float* __restrict__ src, int rows, int cols, int ld, float* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * ld; i += gridDim.x * blockDim.x) {
    const int r = i / ld, c = i - r * ld;
    dst[i] = c < cols ? src[r * cols + c] : 0.f;
  }
}
// dst[c][r] = src[r][c] (32 x 32 tiles through LDS): the hidden layers' weight blocks in the K-contiguous ("NT") layout the
// persistent GEMM's delta products run fastest with (r06)
__global__ __launch_bounds__(256) void k_transpose(const float* __restrict__ src, int rows, int cols, float* __restrict__ dst) {
  __shared__ float tile[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    tile[ty + 8 * i][tx] = (r < rows && c < cols) ? src[(int64_t)r * cols + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (c < cols && r < rows) dst[(int64_t)c * rows + r] = tile[tx][ty + 8 * i];
  }
}
__global__ void k_unpad_rows(const float* __restrict__ src, int rows, int cols, int ld, float* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += gridDim.x * blockDim.x) {
    const int r = i / cols, c = i - r * cols;
    dst[i] = src[r * ld + c];
  }
}

// per-sample likelihood head (mean_LL / likelihood_ratio / mean_kl / CPI surrogate).
// mode 0 (VPG): writes d3 = out_scale * adv*LR/N * (a-mu)/sigma^2, partial sums [surr, count, gls(m)...]
// mode 2 (EVAL): partial sums [surr, kl]
// part: [gridDim.x][2 + MPH] doubles
constexpr int MPH = 64;   // max action dim of the layer-wise head
// r06: ONE pass with the actions on the lanes.  The r01-r05 kernel gave every thread a sample and walked its m actions in a loop
// (rows of m floats per thread: uncoalesced) -- and, to keep the log_std gradients out of a dynamically indexed register array,
// it repeated the WHOLE pass over the batch once per four actions: 7 passes at configs[4]'s 28 actions, 2.27 ms per launch for
// 0.45 GB (K1 and K3 of every update: 4.5 of 226 ms).  Now a wave takes one sample (m > 32) or two (a lane half each) per step: lane a
// holds action a's element of the row (coalesced loads / stores), the sums over the actions are wave reductions (DPP row sums +
// v_permlane16_swap / v_permlane32_swap: no LDS), and lane a keeps d log_std[a] in ONE fp64 register for the whole launch.
// Per element the arithmetic is the old kernel's (the same divisions); the sums over the actions are trees instead of chains, and the
// likelihood ratio is formed from the per-action DIFFERENCE of the two log-likelihoods (below).
__device__ __forceinline__ float head_sum32(float v) {       // every lane: the sum over its 32-lane half
  v = row16_sum(v);
  auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}
constexpr int HEAD_NT = 1024;                            // 16 waves per workgroup: the pass is latency-bound (a row or two per wave step)
__global__ __launch_bounds__(HEAD_NT) void k_head(int mode, const float* __restrict__ mu, const float* __restrict__ mu_old,
                                              const float* __restrict__ act, const float* __restrict__ adv, int64_t N, int m,
                                              const float* __restrict__ ls_new, const float* __restrict__ ls_old,
                                              const float* __restrict__ osc, float inv_N, float* __restrict__ d3,
                                              double* __restrict__ part) {
  __shared__ double sh[17];
  __shared__ double shg[HEAD_NT / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const bool wide = m > 32;                      // one sample per wave step; else two (lane half = sample)
  const int a = wide ? lane : (lane & 31), sub = wide ? 0 : (lane >> 5), SP = wide ? 1 : 2;
  const bool on = a < m;
  const float lsn_a = on ? ls_new[a] : 0.f, lso_a = on ? ls_old[a] : 0.f;
  const float sgn_a = on ? expf(lsn_a) : 1.f, sgo_a = on ? expf(lso_a) : 1.f;
  const float osc_a = (on && mode == 0) ? osc[a] : 0.f;
  const float dkl = 2.0f * sgn_a * sgn_a + 1e-8f;
  float sumn = 0.f, sumo = 0.f;
  for (int k = 0; k < m; ++k) { sumn += ls_new[k]; sumo += ls_old[k]; }
  auto asum = [&](float v) { v = head_sum32(v); return wide ? half_sum(v) : v; };
  double s_surr = 0.0, s_b = 0.0, gl = 0.0;
  const int64_t nw = (int64_t)gridDim.x * nwv;
  for (int64_t i0 = ((int64_t)blockIdx.x * nwv + wave) * SP; i0 < N; i0 += nw * SP) {
    const int64_t i = i0 + sub;
    const bool row = i < N, ok = on && row;
    const int64_t e = ok ? i * m + a : 0;
    const float x = act[e], mn = mu[e];
    const float zn = ok ? (x - mn) / sgn_a : 0.f;
    // LL_new - LL_old = sum_a -0.5 (zn - zo)(zn + zo) - (sum log_std_new - sum log_std_old): the DIFFERENCE per action, summed --
    // not two sums of magnitude ~m/2 + |sum log_std| subtracted afterwards (their fp32 rounding, ~|LL| x 6e-8, went straight into
    // the likelihood ratio: the old != new gradients sat 5e-6..1.3e-5 from the fp64 oracle because of it)
    float dll = 0.f, kl = 0.f;
    if (mu_old) {
      const float mo = mu_old[e];
      const float zo = ok ? (x - mo) / sgo_a : 0.f;
      dll = asum(-0.5f * (zn - zo) * (zn + zo)) - (sumn - sumo);
      const float Nr = (mo - mn) * (mo - mn) + sgo_a * sgo_a - sgn_a * sgn_a;
      kl = asum(ok ? Nr / dkl + lsn_a - lso_a : 0.f);
    }
    const float LR = expf(dll), ad = adv[row ? i : 0];
    if (a == 0 && row) { s_surr += (double)(LR * ad); s_b += (mode == 0) ? 1.0 : (double)kl; }
    if (mode == 0 && ok) {
      const float w = ad * LR * inv_N;
      d3[e] = osc_a * (w * zn / sgn_a);
      gl += (double)(w * (zn * zn - 1.0f));
    }
  }
  shg[wave][lane] = gl;
  __syncthreads();
  if (mode == 0 && (int)threadIdx.x < m) {       // fixed order: waves, then the two lane halves
    double t = 0.0;
    for (int w = 0; w < nwv; ++w)
      for (int h = 0; h < SP; ++h) t += shg[w][h * 32 + threadIdx.x];
    part[(size_t)blockIdx.x * (2 + MPH) + 2 + threadIdx.x] = t;
  }
  s_surr = block_sum(s_surr, sh);
  s_b = block_sum(s_b, sh);
  if (threadIdx.x == 0) { part[(size_t)blockIdx.x * (2 + MPH)] = s_surr; part[(size_t)blockIdx.x * (2 + MPH) + 1] = s_b; }
}

// ---- minibatch losses of the torch-optimizer paths, one block per minibatch ----
// loss 0: MSE(mu, a)            torch.nn.MSELoss, mean over B*m elements        behavior_cloning.py:96-105
// loss 1: -mean LL(a | mu, s)   mean_LL of gaussian_mlp.py:99-115               behavior_cloning.py:83-94
// loss 2: -mean min(LR adv, clamp(LR, 1-c, 1+c) adv), LR = exp(LL - LL_old)     ppo_clip.py:49-56
// writes d3 = dLoss/d(pre-affine output) (B x m), gls = dLoss/dlog_std (m) and the loss value.
// rows: gathered minibatch (mu, mu_old, act, adv are B-row blocks)
__global__ __launch_bounds__(256) void k_minibatch_head(int loss, const float* __restrict__ mu, const float* __restrict__ mu_old,
                                                        const float* __restrict__ act, const float* __restrict__ adv, int B, int m,
                                                        const float* __restrict__ ls, const float* __restrict__ ls_old,
                                                        const float* __restrict__ osc, float clip, float* __restrict__ d3,
                                                        float* __restrict__ gls, double* __restrict__ loss_out) {
  __shared__ double sh[17];
  __shared__ float sg[MPH], sgo[MPH], lsn[MPH], lso[MPH], oscs[MPH];
  __shared__ double glacc[MPH];
  if (threadIdx.x < m) {
    lsn[threadIdx.x] = ls[threadIdx.x]; sg[threadIdx.x] = expf(ls[threadIdx.x]);
    lso[threadIdx.x] = ls_old ? ls_old[threadIdx.x] : 0.f; sgo[threadIdx.x] = ls_old ? expf(ls_old[threadIdx.x]) : 1.f;
    oscs[threadIdx.x] = osc[threadIdx.x];
    glacc[threadIdx.x] = 0.0;
  }
  __syncthreads();
  const float invB = 1.0f / (float)B;
  double lacc = 0.0;
  float sumn = 0.f, sumo = 0.f;
  for (int a = 0; a < m; ++a) { sumn += lsn[a]; sumo += lso[a]; }
  const float c = 0.5f * (float)m * 1.8378770664093453f;
  // per-row weight w: dLoss/dLL of the row (MLE: -1/B; PPO: -adv LR mask / B)
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    if (loss == 0) {
      for (int a = 0; a < m; ++a) {
        const float e = mu[i * m + a] - act[i * m + a];
        d3[i * m + a] = oscs[a] * (2.0f * e * invB / (float)m);
        lacc += (double)e * (double)e;
      }
    } else {
      float lln = 0.f, llo = 0.f;
      for (int a = 0; a < m; ++a) {
        const float x = act[i * m + a];
        const float zn = (x - mu[i * m + a]) / sg[a];
        lln = fmaf(-0.5f * zn, zn, lln);
        if (loss == 2) { const float zo = (x - mu_old[i * m + a]) / sgo[a]; llo = fmaf(-0.5f * zo, zo, llo); }
      }
      lln = lln - sumn - c;
      float w;
      if (loss == 1) { w = -invB; lacc += (double)lln; }
      else {
        llo = llo - sumo - c;
        const float LR = expf(lln - llo), ad = adv[i];
        const float s1 = LR * ad, s2 = fminf(fmaxf(LR, 1.0f - clip), 1.0f + clip) * ad;
        lacc += (double)fminf(s1, s2);
        const bool inside = (LR >= 1.0f - clip) && (LR <= 1.0f + clip);
        // d min(s1, s2)/dLR: adv where the unclipped branch is (co-)active; ties inside the clip range add up to adv
        w = (inside || s1 < s2) ? -ad * LR * invB : 0.f;
      }
      for (int a = 0; a < m; ++a) {
        const float zn = (act[i * m + a] - mu[i * m + a]) / sg[a];
        d3[i * m + a] = oscs[a] * (w * zn / sg[a]);                  // dLL/dmu = z / sigma
      }
    }
  }
  // dLoss/dlog_std[a] = sum_rows w (z^2 - 1): one fixed-order block reduction per action
  if (loss != 0) {
    for (int a = 0; a < m; ++a) {
      double g = 0.0;
      for (int i = threadIdx.x; i < B; i += blockDim.x) {
        float lln = 0.f, llo = 0.f, w;
        if (loss == 1) w = -invB;
        else {
          for (int b = 0; b < m; ++b) {
            const float x = act[i * m + b];
            const float zn = (x - mu[i * m + b]) / sg[b];
            lln = fmaf(-0.5f * zn, zn, lln);
            const float zo = (x - mu_old[i * m + b]) / sgo[b]; llo = fmaf(-0.5f * zo, zo, llo);
          }
          const float LR = expf((lln - sumn - c) - (llo - sumo - c)), ad = adv[i];
          const float s1 = LR * ad, s2 = fminf(fmaxf(LR, 1.0f - clip), 1.0f + clip) * ad;
          const bool inside = (LR >= 1.0f - clip) && (LR <= 1.0f + clip);
          w = (inside || s1 < s2) ? -ad * LR * invB : 0.f;
        }
        const float z = (act[i * m + a] - mu[i * m + a]) / sg[a];
        g += (double)(w * (z * z - 1.0f));
      }
      g = block_sum(g, sh);
      if (threadIdx.x == 0) gls[a] = (float)g;
    }
  }
  lacc = block_sum(lacc, sh);
  if (threadIdx.x == 0 && loss_out) {
    if (loss == 0) loss_out[0] = lacc / ((double)B * (double)m);
    else loss_out[0] = -lacc / (double)B;
  }
}

// rows idx[0..B) of the batch -> contiguous minibatch blocks
__global__ void k_gather_minibatch(const float* __restrict__ obs, const float* __restrict__ act, const float* __restrict__ adv,
                                   const int32_t* __restrict__ idx, int B, int n, int m, float* __restrict__ Xb,
                                   float* __restrict__ Ab, float* __restrict__ advb) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, T = gridDim.x * blockDim.x;
  for (int i = t; i < B * n; i += T) { const int r = i / n, c = i - r * n; Xb[i] = obs[(int64_t)idx[r] * n + c]; }
  for (int i = t; i < B * m; i += T) { const int r = i / m, c = i - r * m; Ab[i] = act[(int64_t)idx[r] * m + c]; }
  if (adv) for (int i = t; i < B; i += T) advb[i] = adv[idx[i]];
}

// FVP head: d3 = out_scale * D * mudot / N,  D = 2/(2 sigma^2 + 1e-8)   (in place on mudot)
__global__ void k_fvp_head(float* __restrict__ mudot, int64_t N, int m, const float* __restrict__ ls,
                           const float* __restrict__ osc, float inv_N) {
  const int64_t tot = N * m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
    int a = (int)(i % m);
    float s = expf(ls[a]);
    float Dk = 2.0f / (2.0f * s * s + 1e-8f);
    mudot[i] = osc[a] * (Dk * mudot[i] * inv_N);
  }
}

// General (theta_new != theta_old) KL Hessian head, per sample and action j  (gaussian_mlp.py:135-145):
//   e = mu_n - mu_o, u = sigma_n^2, D = 2u + 1e-8
//   d3  = out_scale * (2 e / D) / N                                  first-order cotangent on the pre-affine output
//   Rd3 = out_scale * ((2/D) mudot + c_ms v_s) / N,  c_ms = -8 e u / D^2
//   hs_j += (c_ms mudot + g2 v_s) / N,  g2 = -(1e-8 + 2A) 4u (1e-8 - 2u) / D^3,  A = e^2 + sigma_o^2
// mudot (in: post-affine tangent of mu) is overwritten with Rd3; part: [gridDim.x][MPH] doubles.
__global__ __launch_bounds__(256) void k_hvp_head(const float* __restrict__ mu, const float* __restrict__ mu_old,
                                                  float* __restrict__ mudot, float* __restrict__ d3, int64_t N, int m,
                                                  const float* __restrict__ ls_new, const float* __restrict__ ls_old,
                                                  const float* __restrict__ vs, const float* __restrict__ osc, float inv_N,
                                                  double* __restrict__ part) {
  __shared__ double sh[17];
  for (int a = 0; a < m; ++a) {
    const float sn = expf(ls_new[a]), so = expf(ls_old[a]);
    const float u = sn * sn, D = 2.0f * u + 1e-8f, va = vs[a], oa = osc[a];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
      const int64_t o = i * m + a;
      const float e = mu[o] - mu_old[o], md = mudot[o];
      const float cms = -8.0f * e * u / (D * D);
      const float A2 = e * e + so * so;
      const float g2 = -(1e-8f + 2.0f * A2) * 4.0f * u * (1e-8f - 2.0f * u) / (D * D * D);
      d3[o] = oa * (2.0f * e / D) * inv_N;
      mudot[o] = oa * ((2.0f / D) * md + cms * va) * inv_N;
      acc += (double)((cms * md + g2 * va) * inv_N);
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * MPH + a] = acc;
  }
}
__global__ void k_reduce_hs(const double* __restrict__ part, int G, int m, float* __restrict__ out) {
  __shared__ double sh[17];
  for (int a = 0; a < m; ++a) {
    double t = 0.0;
    for (int g = threadIdx.x; g < G; g += blockDim.x) t += part[(size_t)g * MPH + a];
    t = block_sum(t, sh);
    if (threadIdx.x == 0) out[a] = (float)t;
  }
}
// p <- p * (1 - y^2)
__global__ void k_scale_dtanh(float* __restrict__ p, const float* __restrict__ y, int64_t cnt) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
    float yy = y[i];
    p[i] *= fmaf(-yy, yy, 1.0f);
  }
}

// column sums of a (N x h) matrix, split over row ranges: part[z][h]
__global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ D, int64_t N, int h, int64_t ld, float* __restrict__ part) {
  __shared__ float sh[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  int64_t chunk = (N + gridDim.y - 1) / gridDim.y;
  int64_t lo = blockIdx.y * chunk, hi = min(N, lo + chunk);
  float a = 0.f;
  if (c < h)
    for (int64_t r = lo + rg; r < hi; r += 4) a += D[r * ld + c];
  sh[rg][threadIdx.x & 63] = a;
  __syncthreads();
  if (rg == 0 && c < h) part[(size_t)blockIdx.y * h + c] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// column sums of a narrow (N x h, h <= 32) matrix: every thread owns whole rows (contiguous h floats), so a wave
// reads one contiguous block of memory per step; part[blockIdx.x][h], fixed order
template <int HMAX>
__global__ __launch_bounds__(256) void k_colsum_narrow(const float* __restrict__ D, int64_t N, int h, float* __restrict__ part) {
  __shared__ float sh[4][HMAX];
  float acc[HMAX];
#pragma unroll
  for (int c = 0; c < HMAX; ++c) acc[c] = 0.f;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) {
    const float* row = D + r * h;
#pragma unroll
    for (int c = 0; c < HMAX; ++c) if (c < h) acc[c] += row[c];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < HMAX; ++c) {
    float v = acc[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) sh[w][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < h) part[(size_t)blockIdx.x * h + threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

__global__ void k_reduce_head(const double* __restrict__ part, int G, int m, int mode, double* __restrict__ scal, float* __restrict__ gls) {
  __shared__ double sh[17];
  for (int k = 0; k < 2 + ((mode == 0) ? m : 0); ++k) {
    double a = 0.0;
    for (int g = threadIdx.x; g < G; g += blockDim.x) a += part[(size_t)g * (2 + MPH) + k];
    a = block_sum(a, sh);
    if (threadIdx.x == 0) {
      if (k < 2) scal[k] = a;
      else gls[k - 2] = (float)a;
    }
  }
  if (threadIdx.x == 0) { scal[2] = (mode == 0) ? scal[1] : 0.0; scal[3] = 0.0; }
}

// log_std block of the FVP: frac * c(sigma) * v_s   
__global__ void k_fvp_logstd(const float* __restrict__ ls, const float* __restrict__ vs, int m, float frac, float* __restrict__ out) {
  int a = threadIdx.x;
  if (a >= m) return;
  float s = expf(ls[a]);
  float u = s * s, den = 2.0f * u + 1e-8f;
  out[a] = frac * (16.0f * u * u / (den * den) - 4.0f * u / den) * vs[a];
}

// A grow-only block of device memory that frees itself.  ensure() keeps the block when it is large enough, else frees it and
// allocates anew: the contents are scratch across a growth.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;                    // elements
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~DevBuf() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  int ensure(size_t count) {         // 0, or 2: out of memory
    if (count <= cap) return 0;
    release();
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) { p = nullptr; return 2; }
    cap = count;
    return 0;
  }
  operator T*() const { return p; }
};

// The workspace of one context's layer-wise path: buffers, what is valid in them, and the operations.
//
// What is cached, and what drops it:
//   H (hidden activations of theta_new on rows [0, fwd_rows) of the bound batch), Wt (the hidden weight blocks of `wt_theta`,
//   transposed by the forward pass that filled H) -- valid while fwd_valid.
//   mu as surr_vpg left it at old == new (the OLD policy's outputs for rows [0, mu_rows) of mu_obs) -- valid while mu_valid; the
//   context's lw_old_ok says whether theta_old / its transform are still the ones it was computed from.
//   * a new batch drops both (reserve; on the fused path, which reserves nothing here, mjx_bind_batch calls invalidate);
//   * new parameters (invalidate) drop H / Wt and leave mu to lw_old_ok;
//   * a binding narrowed to a prefix of the rows (narrow) keeps both: the prefix of either cache is valid;
//   * surr_vpg refills H (and mu, which is the old policy's only at old == new); fvp refills H when it is not valid, and then
//     drops mu, which the refill overwrites; hvp_general always refills H and drops mu;
//   * every forward pass that is not cached overwrites Xn (its own transform) and T: eval drops fwd_valid whenever it runs a
//     network, and drops mu unless it reused it; mjx_policy_forward (forward_scratch) drops fwd_valid and leaves mu alone;
//   * the minibatch trainer (MinibatchWS) works in a workspace of its own and touches nothing here.
struct LayerwiseWS {
  int n = 0, m = 0;
  std::vector<int> sizes;            // n, h..., m
  std::vector<int64_t> oW, ob;       // offsets in the flat vector
  int64_t oS = 0, d = 0;
  int64_t cap = 0;                   // rows allocated
  DevBuf<float> Xn;                  // normalised obs (N x ldx(): rows padded with zeros to a multiple of 4 floats)
  DevBuf<float> V1p, G1p, W1p;       // first-layer direction / gradient / weight blocks with rows padded the same way (only when ldx() != n)
  // r06: W_l^T of the hidden layers l >= 1 (made by the forward pass that fills the activation cache, from the same theta): the
  // delta product delta_l W_l then has its B operand K-contiguous like the tangent products, i.e. runs as k_gemm_p<0, EPI_BACK>
  // (0.75-0.76 of the fp32-MFMA peak) instead of <1, EPI_BACK> (0.67: one ds_read_b32 per k-step and column instead of a
  // ds_read_b128 per four).  MJX_LW_WT=0: the weights as they lie.
  std::vector<DevBuf<float>> Wt;
  const float* wt_theta = nullptr;
  bool wt_eligible(int l) const { return l >= 1 && l < nL() && sizes[l + 1] >= 64 && (sizes[l + 1] % 32) == 0 && (sizes[l] % 4) == 0 && sizes[l] > 32; }
  // (up to 32 features: whole 16-byte granules; beyond: whole 128-byte k-tiles, so that every k-tile segment of a row is one
  //  cache line and the first layer needs no K tail -- 376 -> 384, 39 -> 64)
  int ldx() const { return n <= 32 ? ((n + 3) & ~3) : ((n + 31) & ~31); }
  int ld_in(int l) const { return l == 0 ? ldx() : sizes[l]; }   // row stride of layer l's input activations
  std::vector<DevBuf<float>> H;      // hidden activations of the NEW net (cached)
  std::vector<DevBuf<float>> T;      // tangent / delta buffers per hidden layer; scratch activations of a forward pass that is not cached
  DevBuf<float> mu, mu2, d3;         // (N x m)
  std::vector<DevBuf<float>> P, RD;  // general-HVP extras: pre-activation cotangents / R-deltas (lazy)
  DevBuf<float> rd3;
  DevBuf<float> part;                // split-K partials
  // MJX_LW_OVERLAP=1 (experiment, r05): the weight gradient of layer l on a side stream beside the delta product towards layer
  // l - 1 (both only read delta_l): its own column-sum workspace, one event fork / join per layer
  DevBuf<float> cpart2;
  hipStream_t side = nullptr; hipEvent_t ev_a = nullptr, ev_b = nullptr;
  DevBuf<double> hpart;              // head partials
  bool fwd_valid = false;
  int64_t fwd_rows = 0;
  bool mu_valid = false; int64_t mu_rows = 0; const float* mu_obs = nullptr;
  int nL() const { return (int)sizes.size() - 1; }   // number of affine layers

  void init(int n_, int m_, const std::vector<int>& hid) {
    n = n_; m = m_;
    sizes.clear(); sizes.push_back(n); for (int h : hid) sizes.push_back(h); sizes.push_back(m);
    oW.clear(); ob.clear();
    int64_t k = 0;
    for (int l = 0; l < nL(); ++l) { oW.push_back(k); k += (int64_t)sizes[l] * sizes[l + 1]; ob.push_back(k); k += sizes[l + 1]; }
    oS = k; d = k + m;
    H = std::vector<DevBuf<float>>(hid.size()); T = std::vector<DevBuf<float>>(hid.size());
    P = std::vector<DevBuf<float>>(hid.size()); RD = std::vector<DevBuf<float>>(hid.size());
    Wt = std::vector<DevBuf<float>>(sizes.size());
  }
  void invalidate() { fwd_valid = false; }
  void narrow(int64_t N) { if (N > fwd_rows) fwd_valid = false; }      // fewer rows of the same batch: the prefix of the cache stays valid
  void release() {                   // back to the state init() left: every buffer frees itself
    if (side) (void)hipStreamDestroy(side);
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
    if (sizes.empty()) { *this = LayerwiseWS(); return; }
    const int n_ = n, m_ = m;
    const std::vector<int> hid(sizes.begin() + 1, sizes.end() - 1);
    *this = LayerwiseWS();
    init(n_, m_, hid);
  }
  static constexpr int HEAD_G = 512;
  int reserve(int64_t N) {           // a new batch of N rows: nothing cached applies
    fwd_valid = false; mu_valid = false;
    if (m > MPH) return -3;
    if (N <= cap) return 0;
    const size_t newcap = (size_t)((N + 127) / 128 * 128);       // whole 128-row tiles: the persistent GEMM (lw_gemm_p.h) reads / writes the padding rows
    release();
    if (Xn.ensure(newcap * ldx())) return 2;
    (void)hipMemset(Xn, 0, newcap * ldx() * 4);
    if (ldx() != n && nL() >= 1)                                // padded first-layer blocks (direction / gradient)
      if (V1p.ensure((size_t)sizes[1] * ldx()) || G1p.ensure((size_t)sizes[1] * ldx()) || W1p.ensure((size_t)sizes[1] * ldx())) return 2;
    for (size_t l = 0; l < H.size(); ++l)
      if (H[l].ensure(newcap * sizes[l + 1]) || T[l].ensure(newcap * sizes[l + 1])) return 2;
    for (int l = 1; l < nL(); ++l)
      if (wt_eligible(l) && Wt[l].ensure((size_t)sizes[l] * sizes[l + 1])) return 2;
    if (mu.ensure(newcap * m) || mu2.ensure(newcap * m) || d3.ensure(newcap * m) || hpart.ensure((size_t)HEAD_G * (2 + MPH))) return 2;
    cap = (int64_t)newcap;
    return 0;
  }
  int ensure_rows(int64_t N) { return cap < N ? reserve(N) : 0; }     // room for N rows; a growth drops everything cached

  // forward pass of one parameter set into `out` (N x m).  cache: the hidden activations go to H and this theta's hidden weight
  // blocks are transposed into Wt (the caller sets fwd_valid); otherwise they are scratch in T
  void forward(const float* theta, const float* tr, const float* obs, int64_t N, bool cache, float* out, hipStream_t st, const LwSwitches& sw) {
    std::vector<DevBuf<float>>& acts = cache ? H : T;
    hipLaunchKernelGGL(k_normalize, dim3(ew_grid(N * ldx())), dim3(256), 0, st, obs, N, n, ldx(), tr, Xn.p);
    if (cache) {
      wt_theta = nullptr;
      if (LwSwitches::wt()) {
        for (int l = 1; l < nL(); ++l)
          if (Wt[l]) hipLaunchKernelGGL(k_transpose, dim3((sizes[l] + 31) / 32, (sizes[l + 1] + 31) / 32), dim3(256), 0, st, theta + oW[l], sizes[l + 1], sizes[l], Wt[l].p);
        wt_theta = theta;
      }
    }
    const float* in = Xn;
    for (int l = 0; l < nL(); ++l) {
      const bool last = (l == nL() - 1);
      const float* W = theta + oW[l];
      int K = sizes[l];
      if (l == 0 && !last && ldx() != n && W1p != nullptr) {       // padded rows: K = ldx() (the pad columns of Xn and of W1p are zero)
        hipLaunchKernelGGL(k_pad_rows, dim3(ew_grid((int64_t)sizes[1] * ldx())), dim3(256), 0, st, theta + oW[0], sizes[1], n, ldx(), W1p.p);
        K = ldx(); W = W1p;
      }
      GemmArgs g = gemm_nt((int)N, sizes[l + 1], K, in, ld_in(l), W, K, last ? out : acts[l].p, last ? EPI_BIAS_AFFINE : EPI_BIAS_TANH);
      g.bias = theta + ob[l];
      g.osc = tr + 2 * n + m; g.osh = tr + 2 * n;
      g.rows_padded = last ? 0 : 1;                  // hidden activations live in workspace blocks (H / T: whole 128-row tiles)
      lw_launch_gemm(g, 1, st, sw);
      in = g.C;
    }
  }
  // mjx_policy_forward: any parameters on any rows, the hidden activations of the bound policy are overwritten (scratch)
  hipError_t forward_scratch(const float* theta, const float* tr, const float* obs, int64_t N, float* out, hipStream_t st) {
    invalidate();
    forward(theta, tr, obs, N, false, out, st, LwSwitches::read());
    return lw_status();
  }

  // backward from d3 (N x m cotangent on the pre-affine output) into grad (flat, W and b blocks).
  // Bias gradients (column sums of delta_l) come out of the GEMM that produces delta_l (per-block column sums in its
  // epilogue, reduced in a fixed order); only the top delta (d3, written by the head kernel) needs its own pass.
  // (l_start / delta0: continue below the output layer when fvp_head() already produced that layer's gradients, the
  // delta of the last hidden layer and its column sums)
  int backward(const float* theta, int64_t N, float* grad, hipStream_t st, const LwSwitches& sw, int l_start = -1, const float* delta0 = nullptr) {
    const float* delta = delta0 ? delta0 : d3.p;
    bool bias_done = delta0 != nullptr;
    const bool overlap = sw.overlap && N >= 65536;
    if (overlap && !side) {
      if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ev_a, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&ev_b, hipEventDisableTiming) != hipSuccess) return 2;
    }
    const int ncu = cu_count();
    hipStream_t main_st = st;
    if (overlap) { (void)hipEventRecord(ev_a, main_st); (void)hipStreamWaitEvent(side, ev_a, 0); }     // delta of the top layer is ready on the caller's stream
    for (int l = (l_start >= 0 ? l_start : nL() - 1); l >= 0; --l) {
      if (overlap) st = side;                        // this layer's weight gradient (and its reductions) go to the side stream
      const int ho = sizes[l + 1], hi_ = sizes[l];
      const float* in = (l == 0) ? Xn : H[l - 1];
      // weight gradient: gW[ho x hi] = delta^T (ho x N) * in (N x hi), split over samples
      const bool narrow = ho <= 32;                 // action head: compute gW^T (hi x ho) so the padding goes to 32 columns, not 128 rows
      const int rowblocks = (int)((N + 127) / 128);      // of the delta GEMM below (its column sums; sample-major launches use 128-row tiles)
      const int splits = wgrad_splits(N, ho, hi_, narrow, sw, ncu);
      const int csplits = 256;
      const int rsplits = 64;                      // second-stage split of the per-row-block column sums
      // first layer of an observation width that is not a multiple of 4: the gradient block is formed with padded rows
      // (ldx() columns: 16-byte operand granules of Xn, the pad column is zero) and compacted afterwards
      const bool padw = (l == 0) && !narrow && ldx() != n && G1p != nullptr;
      const int wN = padw ? ldx() : hi_;
      if (part.ensure((size_t)((int64_t)splits * ho * wN + (int64_t)csplits * ho + (int64_t)rowblocks * hi_ + (int64_t)rsplits * hi_))) return 2;
      float* wdst = padw ? G1p.p : grad + oW[l];
      // (a single split / row block -- minibatches -- writes the gradient blocks directly: no reduction launches)
      lw_launch_gemm(gemm_wgrad((int)N, ho, wN, delta, in, ld_in(l), (splits == 1) ? wdst : part.p, narrow), splits, st, sw);
      if (splits > 1) lw_reduce_split(part, splits, (int64_t)ho * wN, wdst, st, sw);
      if (padw) hipLaunchKernelGGL(k_unpad_rows, dim3(ew_grid((int64_t)ho * hi_)), dim3(256), 0, st, G1p.p, ho, hi_, wN, grad + oW[l]);
      float* bpart = part + (int64_t)splits * ho * wN;
      float* cpart = bpart + (int64_t)csplits * ho;
      if (overlap) {
        // the delta product below runs on the caller's stream beside this layer's weight gradient: its column-sum partials get a
        // block of their own (the next layer's gradient slabs on the side stream may grow over `cpart`)
        if (cpart2.ensure((size_t)((int64_t)rowblocks * hi_ + (int64_t)rsplits * hi_))) return 2;
        cpart = cpart2;
      }
      if (!bias_done) {
        const int cs = (N <= 4096) ? 1 : csplits;
        float* dst = (cs == 1) ? grad + ob[l] : bpart;
        if (ho <= 32) hipLaunchKernelGGL(k_colsum_narrow<32>, dim3(cs), dim3(256), 0, st, delta, N, ho, dst);
        else hipLaunchKernelGGL(k_colsum, dim3((ho + 63) / 64, cs), dim3(256), 0, st, delta, N, ho, (int64_t)ho, dst);
        if (cs > 1)
          hipLaunchKernelGGL(k_reduce_partials, dim3((ho + 15) / 16), dim3(256), 0, st, bpart, cs, ho, grad + ob[l],
                             (const float*)nullptr, (const float*)nullptr, 0, 0.f);
      }
      if (overlap) st = main_st;                     // ... the delta product towards the layer below stays on the caller's stream
      if (l > 0) {
        // delta_{l} = (delta_{l+1} W_l) (1 - H_{l-1}^2)   -> T[l-1]   (+ its column sums = grad b_{l-1})
        const bool wt = Wt[l] && wt_theta == theta && N >= 2 * GP_BM;           // W_l^T: B(k, j) = Wt[j][k]
        GemmArgs b = gemm_delta((int)N, ho, hi_, delta, wt ? Wt[l].p : theta + oW[l], wt, T[l - 1], H[l - 1], EPI_BACK);
        b.rows_padded = (delta != d3) ? 1 : 0;         // (delta of a hidden layer lives in T[l]; the top delta d3 has no padding rows)
        b.colsum = (rowblocks == 1) ? grad + ob[l - 1] : cpart;
        lw_launch_gemm(b, 1, st, sw);
        if (rowblocks > 1024) {
          // thousands of row blocks (3 907 at 500 k samples): 16..32 workgroups walking them took 100-200 us per layer;
          // sum them in 64 row ranges first (k_colsum: 64 x hi/64 workgroups), then the 64 partial rows -- fixed order
          float* rpart = cpart + (int64_t)rowblocks * hi_;
          hipLaunchKernelGGL(k_colsum, dim3((hi_ + 63) / 64, rsplits), dim3(256), 0, st, cpart, (int64_t)rowblocks, hi_, (int64_t)hi_, rpart);
          hipLaunchKernelGGL(k_reduce_partials, dim3((hi_ + 15) / 16), dim3(256), 0, st, rpart, rsplits, hi_, grad + ob[l - 1],
                             (const float*)nullptr, (const float*)nullptr, 0, 0.f);
        } else if (rowblocks > 1)
          hipLaunchKernelGGL(k_reduce_partials, dim3((hi_ + 15) / 16), dim3(256), 0, st, cpart, rowblocks, hi_, grad + ob[l - 1],
                             (const float*)nullptr, (const float*)nullptr, 0, 0.f);
        bias_done = true;
        delta = T[l - 1];
        if (overlap) { (void)hipEventRecord(ev_a, main_st); (void)hipStreamWaitEvent(side, ev_a, 0); }   // the next layer's gradient needs this delta
      }
    }
    if (overlap) { (void)hipEventRecord(ev_b, side); (void)hipStreamWaitEvent(main_st, ev_b, 0); }      // join: the gradients are complete on the caller's stream
    return lw_status() == hipSuccess ? 0 : 1;
  }

  int surr_vpg(const float* obs, const float* act, const float* adv, int64_t N, int64_t Ng, const float* th_new,
               const float* th_old, const float* tr_new, const float* tr_old, int old_is_new, float* grad, double* scal,
               hipStream_t st) {
    if (N > cap) return 1;
    const LwSwitches sw = LwSwitches::read();
    const float* mo = nullptr;
    if (!old_is_new) {          // old net first (its hidden activations are scratch in T)
      forward(th_old, tr_old, obs, N, false, mu2, st, sw);
      mo = mu2;
    }
    forward(th_new, tr_new, obs, N, true, mu, st, sw);
    fwd_valid = true; fwd_rows = N;
    mu_valid = old_is_new != 0; mu_rows = N; mu_obs = obs;
    hipLaunchKernelGGL(k_head, dim3(HEAD_G), dim3(HEAD_NT), 0, st, 0, mu.p, mo, act, adv, N, m, th_new + oS, th_old + oS,
                       tr_new + 2 * n + m, (float)(1.0 / (double)Ng), d3.p, hpart.p);
    hipLaunchKernelGGL(k_reduce_head, dim3(1), dim3(256), 0, st, hpart.p, HEAD_G, m, 0, scal, grad + oS);
    return backward(th_new, N, grad, st, sw);
  }

  // Tangent (R-forward) pass of direction v at theta, over the cached H:  T_l = (in V_l^T + T_{l-1} W_l^T + c_l)(1 - H_l^2) for
  // the hidden layers.  The output layer's product takes its destination, epilogue and epilogue constants from `top`; top ==
  // nullptr leaves it out (fvp_head does that layer).  rows_padded: what the hidden products declare (GemmArgs::rows_padded).
  void tangent(const float* theta, const float* v, int64_t N, int rows_padded, const GemmArgs* top, hipStream_t st, const LwSwitches& sw) {
    const float* tin = nullptr;
    for (int l = 0; l < nL(); ++l) {
      const bool last = (l == nL() - 1);
      if (last && !top) break;
      const float* in = (l == 0) ? Xn : H[l - 1];
      const float* V = v + oW[l];
      int K = sizes[l];
      if (l == 0 && ldx() != n && V1p != nullptr) {       // padded rows: K = ldx() (the pad column of Xn and of V1p is zero)
        hipLaunchKernelGGL(k_pad_rows, dim3(ew_grid((int64_t)sizes[1] * ldx())), dim3(256), 0, st, v + oW[0], sizes[1], n, ldx(), V1p.p);
        K = ldx(); V = V1p;
      }
      GemmArgs g = gemm_nt((int)N, sizes[l + 1], K, in, ld_in(l), V, K, last ? top->C : T[l].p, last ? top->epi : (int)EPI_TANGENT);
      if (tin) gemm_nt_pair(g, 1, sizes[l], tin, sizes[l], theta + oW[l], sizes[l]);
      g.bias = v + ob[l];
      if (last) { g.osc = top->osc; g.osh = top->osh; g.ls = top->ls; g.inv_N = top->inv_N; }
      else { g.aux = H[l]; g.ld_aux = sizes[l + 1]; g.rows_padded = rows_padded; }
      lw_launch_gemm(g, 1, st, sw);
      tin = last ? nullptr : T[l].p;
    }
  }

  int fvp(const float* obs, int64_t N, int64_t Ng, const float* theta, const float* tr, const float* v, float* out, hipStream_t st) {
    if (N > cap) return 1;
    const LwSwitches sw = LwSwitches::read();
    if (!fwd_valid || N > fwd_rows) { forward(theta, tr, obs, N, true, mu, st, sw); fwd_valid = true; fwd_rows = N; mu_valid = false; }
    const bool fused = head_fused(theta, v, sw);
    // the output layer's tangent goes straight to d3 = out_scale D mudot / N in the GEMM epilogue (no pass over N x m)
    GemmArgs top{};
    top.C = d3; top.epi = EPI_FVP_HEAD; top.osc = tr + 2 * n + m; top.ls = theta + oS; top.inv_N = (float)(1.0 / (double)Ng);
    tangent(theta, v, N, 1, fused ? nullptr : &top, st, sw);
    hipLaunchKernelGGL(k_fvp_logstd, dim3(1), dim3(64), 0, st, theta + oS, v + oS, m, (float)((double)N / (double)Ng), out + oS);
    if (fused) {
      if (int rc = fvp_head(theta, tr, v, N, Ng, out, st, sw)) return rc;
      return backward(theta, N, out, st, sw, nL() - 2, T[nL() - 2]);
    }
    return backward(theta, N, out, st, sw);
  }

  // the output layer of the product as one pass over the last hidden layer (lw_head.h); MJX_LW_HEAD=0 keeps the generic chain
  // (the pass reads theta / v with 16-byte loads: a direction that is a view at an odd offset of a larger tensor takes the
  //  generic chain instead of failing -- the fast path is an optimisation, not a precondition)
  bool head_fused(const float* theta, const float* v, const LwSwitches& sw) const {
    if (!sw.head || nL() < 2 || m > 32) return false;
    if ((((uintptr_t)theta | (uintptr_t)v) & 15) != 0) return false;
    const int hl = sizes[nL() - 1];
    return (hl % 128) == 0 && hl <= 512 && (oW[nL() - 1] % 4) == 0;
  }
  int fvp_head(const float* theta, const float* tr, const float* v, int64_t N, int64_t Ng, float* out, hipStream_t st, const LwSwitches& sw) {
    const int L = nL() - 1, hl = sizes[L];
    const int ncu = cu_count();
    const int64_t ntile = (N + LH_R - 1) / LH_R;
    const int grid = (int)(ntile < ncu ? ntile : ncu);             // one workgroup per CU (the kernel takes the whole register file: lw_head.h)
    if (part.ensure((size_t)((int64_t)grid * ((int64_t)m * hl + 32 + hl)))) return 2;
    HeadArgs a{};
    a.H = H[L - 1]; a.T = T[L - 1]; a.V3 = v + oW[L]; a.W3 = theta + oW[L]; a.c3 = v + ob[L];
    a.osc = tr + 2 * n + m; a.ls = theta + oS; a.inv_N = (float)(1.0 / (double)Ng);
    a.N = N; a.h = hl; a.m = m;
    a.gw_part = part; a.gb_part = part + (int64_t)grid * m * hl; a.cs_part = a.gb_part + (int64_t)grid * 32;
    auto launch = [&](auto ch) {
      constexpr int CH = decltype(ch)::value;
      void (*const kern)(HeadArgs) = k_lw_head<CH>;
      if (lw_dyn_lds((const void*)kern, lw_head_lds_bytes())) hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lw_head_lds_bytes(), st, a);
    };
    auto launch8 = [&](auto ch) {             // 256 / 512 units: the eight-wave build (two waves per SIMD)
      constexpr int CH = decltype(ch)::value;
      // the delta product's contraction over the actions in ceil(m / 2) steps: 9 (m <= 18: Humanoid's 17), 12 (<= 24), else all 16
      void (*const kern)(HeadArgs) = !sw.head_ktrim ? k_lw_head8<CH, 16> : m <= 18 ? k_lw_head8<CH, 9> : m <= 24 ? k_lw_head8<CH, 12> : k_lw_head8<CH, 16>;
      if (lw_dyn_lds((const void*)kern, lw_head8_lds_bytes())) hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lw_head8_lds_bytes(), st, a);
    };
    // (r06: k_lw_head8 re-bases its buffer resources per row tile -- no 4 GB limit on the blocks any more)
    if (sw.head8 && hl == 256) launch8(std::integral_constant<int, 1>{});
    else if (sw.head8 && hl == 512) launch8(std::integral_constant<int, 2>{});
    else switch (hl / 128) {
      case 1: launch(std::integral_constant<int, 1>{}); break;
      case 2: launch(std::integral_constant<int, 2>{}); break;
      case 3: launch(std::integral_constant<int, 3>{}); break;
      default: launch(std::integral_constant<int, 4>{}); break;
    }
    lw_reduce_split(a.gw_part, grid, (int64_t)m * hl, out + oW[L], st, sw);
    hipLaunchKernelGGL(k_reduce_partials, dim3((m + 15) / 16), dim3(256), 0, st, a.gb_part, grid, m, out + ob[L], (const float*)nullptr,
                       (const float*)nullptr, 0, 0.f);
    hipLaunchKernelGGL(k_reduce_partials, dim3((hl + 15) / 16), dim3(256), 0, st, a.cs_part, grid, hl, out + ob[L - 1], (const float*)nullptr,
                       (const float*)nullptr, 0, 0.f);
    return 0;
  }

  // Exact Hessian-vector product of mean_kl(new, old) wrt theta_new for theta_new != theta_old
  // (npg_cg.py:62-81 in general position, e.g. under input_normalization :101-107):
  // forward + R-forward + backward + R-backward (Pearlmutter), without the damping term.
  int hvp_general(const float* obs, int64_t N, int64_t Ng, const float* th_new, const float* th_old, const float* tr_new,
                  const float* tr_old, const float* v, float* out, hipStream_t st) {
    if (N > cap) return 1;
    const LwSwitches sw = LwSwitches::read();
    const int ncu = cu_count();
    for (size_t l = 0; l < P.size(); ++l)
      if (P[l].ensure((size_t)cap * sizes[l + 1]) || RD[l].ensure((size_t)cap * sizes[l + 1])) return 2;
    if (rd3.ensure((size_t)cap * m)) return 2;
    const float inv_N = (float)(1.0 / (double)Ng);
    forward(th_old, tr_old, obs, N, false, mu2, st, sw);     // old means (hidden activations are scratch)
    forward(th_new, tr_new, obs, N, true, mu, st, sw);
    fwd_valid = true; fwd_rows = N; mu_valid = false;
    // R-forward: T_l = (in V_l^T + T_{l-1} W_l^T + c_l)(1 - H_l^2), rd3 = out_scale (.. + c_L)
    // (its hidden products do not declare padded rows: they take the persistent kernel at whole 128-row tiles only, as they always have)
    GemmArgs top{};
    top.C = rd3; top.epi = EPI_BIAS_AFFINE; top.osc = tr_new + 2 * n + m;
    tangent(th_new, v, N, 0, &top, st, sw);
    hipLaunchKernelGGL(k_hvp_head, dim3(HEAD_G), dim3(256), 0, st, mu.p, mu2.p, rd3.p, d3.p, N, m, th_new + oS, th_old + oS, v + oS,
                       tr_new + 2 * n + m, inv_N, hpart.p);
    hipLaunchKernelGGL(k_reduce_hs, dim3(1), dim3(256), 0, st, hpart.p, HEAD_G, m, out + oS);
    // backward with R: delta (first order) and Rdelta
    const float* dl = d3; const float* rdl = rd3;
    for (int l = nL() - 1; l >= 0; --l) {
      const int ho = sizes[l + 1], hi_ = sizes[l];
      const float* in = (l == 0) ? Xn : H[l - 1];
      const float* tinl = (l == 0) ? nullptr : T[l - 1].p;
      const int splits = wgrad_splits(N, ho, hi_, false, sw, ncu);
      if (part.ensure((size_t)((int64_t)splits * ho * hi_ + (int64_t)splits * ho))) return 2;
      GemmArgs g = gemm_wgrad((int)N, ho, hi_, rdl, in, ld_in(l), part);        // R{gW_l} = Rdelta^T in + delta^T Tin
      if (tinl) gemm_wgrad_pair(g, 1, (int)N, ho, dl, tinl, hi_);
      lw_launch_gemm(g, splits, st, sw);
      lw_reduce_split(part, splits, (int64_t)ho * hi_, out + oW[l], st, sw);
      float* bpart = part + (int64_t)splits * ho * hi_;
      hipLaunchKernelGGL(k_colsum, dim3((ho + 63) / 64, splits), dim3(256), 0, st, rdl, N, ho, (int64_t)ho, bpart);
      hipLaunchKernelGGL(k_reduce_split, dim3(ew_grid(ho)), dim3(256), 0, st, bpart, splits, (int64_t)ho, out + ob[l]);
      if (l > 0) {
        // pre = delta W_l
        lw_launch_gemm(gemm_delta((int)N, ho, hi_, dl, th_new + oW[l], false, P[l - 1], nullptr, EPI_STORE), 1, st, sw);
        // Rdelta_l = (delta V_l + Rdelta W_l)(1-H^2) - 2 H T pre
        GemmArgs b = gemm_delta((int)N, ho, hi_, dl, v + oW[l], false, RD[l - 1], H[l - 1], EPI_RBACK);
        gemm_delta_pair(b, 1, ho, hi_, rdl, th_new + oW[l]);
        b.aux2 = T[l - 1]; b.aux3 = P[l - 1];
        lw_launch_gemm(b, 1, st, sw);
        hipLaunchKernelGGL(k_scale_dtanh, dim3(ew_grid(N * hi_)), dim3(256), 0, st, P[l - 1].p, H[l - 1].p, N * hi_);
        dl = P[l - 1]; rdl = RD[l - 1];
      }
    }
    return lw_status() == hipSuccess ? 0 : 1;
  }

  // old_cached: the caller vouches that theta_old / tr_old / obs are what surr_vpg saw (the one-call updates: nothing outside the
  // library runs between their K1 and their evaluations); old_is_new: theta_new == theta_old as well (DAPG's surr_before)
  int eval(const float* obs, const float* act, const float* adv, int64_t N, const float* th_new, const float* th_old,
           const float* tr_new, const float* tr_old, double* scal, hipStream_t st, bool old_cached = false, bool old_is_new = false) {
    if (N > cap) return 1;
    const bool reuse_on = LwSwitches::old_outputs();
    const LwSwitches sw = LwSwitches::read();
    const float *mnew = mu, *mold = mu2;
    if (reuse_on && old_cached && mu_valid && obs == mu_obs && N <= mu_rows) {
      if (old_is_new) { mnew = mu; mold = nullptr; }                    // LR = 1, KL = 0: no network runs at all; the caches stay
      else {
        forward(th_new, tr_new, obs, N, false, mu2, st, sw);            // (hidden activations are scratch; `mu` keeps the old outputs)
        fwd_valid = false;
        mnew = mu2; mold = mu;
      }
    } else {
      forward(th_old, tr_old, obs, N, false, mu2, st, sw);
      forward(th_new, tr_new, obs, N, false, mu, st, sw);       // hidden activations are scratch here
      fwd_valid = false; mu_valid = false;
    }
    hipLaunchKernelGGL(k_head, dim3(HEAD_G), dim3(HEAD_NT), 0, st, 2, mnew, mold, act, adv, N, m, th_new + oS, th_old + oS,
                       tr_new + 2 * n + m, 0.f, (float*)nullptr, hpart.p);
    hipLaunchKernelGGL(k_reduce_head, dim3(1), dim3(256), 0, st, hpart.p, HEAD_G, m, 2, scal, (float*)nullptr);
    return lw_status() == hipSuccess ? 0 : 1;
  }
};

// The launch-based minibatch trainer's workspace (mjx_policy_minibatch_adam with MJX_NO_POLICY_FIT=1 or a shape the one-launch
// trainer does not hold): a layer-wise workspace of B rows of its own, the gathered minibatch and the gradient.
struct MinibatchWS {
  LayerwiseWS lw;
  DevBuf<float> x, a, adv, grad;     // B x n, B x m, B, d
  int reserve(int B) {
    if (int rc = lw.ensure_rows(B)) return rc;
    return (x.ensure((size_t)B * lw.n) || a.ensure((size_t)B * lw.m) || adv.ensure((size_t)B) || grad.ensure((size_t)lw.d)) ? 2 : 0;
  }
  void release() { lw.release(); x.release(); a.release(); adv.release(); grad.release(); }
  // rows idx[0, B) of the batch -> the gradient of the loss on them at theta, in `grad` (loss: k_minibatch_head)
  int grad_step(int loss, const float* obs, const float* act, const float* advs, const int32_t* idx, int B, const float* theta,
                const float* trn, const float* theta_old, const float* tro, bool old_fwd, float clip, double* loss_out, unsigned ggrid,
                hipStream_t st) {
    const int n = lw.n, m = lw.m;
    const LwSwitches sw = LwSwitches::read();
    hipLaunchKernelGGL(k_gather_minibatch, dim3(ggrid), dim3(256), 0, st, obs, act, (loss == 2) ? advs : (const float*)nullptr, idx, B, n, m,
                       x.p, a.p, adv.p);
    if (old_fwd) lw.forward(theta_old, tro, x, B, false, lw.mu2, st, sw);          // old policy on the minibatch (activations are scratch)
    lw.forward(theta, trn, x, B, true, lw.mu, st, sw);
    hipLaunchKernelGGL(k_minibatch_head, dim3(1), dim3(256), 0, st, loss, lw.mu.p, (loss == 2) ? (old_fwd ? lw.mu2.p : lw.mu.p) : (const float*)nullptr, a.p,
                       adv.p, B, m, theta + lw.oS, (loss == 2) ? theta_old + lw.oS : (const float*)nullptr, trn + 2 * n + m,
                       clip, lw.d3.p, grad + lw.oS, loss_out);
    return lw.backward(theta, B, grad, st, sw);
  }
};

}  // namespace mjx
