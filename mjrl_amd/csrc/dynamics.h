// dynamics.h -- learned-dynamics kernels for model-based NPG (mjrl/algos/model_accel/):
//
//   k_dyn_forward    batched DynamicsNet / RewardNet forward, K ensemble members in one launch
//                    (nn_dynamics.py:230-244, 313-327): input normalisation over the concatenated input, ReLU / tanh hidden
//                    layers, output affine, mask (out_scale >= 1e-8) and residual (+ s), each switchable (DYN_* flags)
//   k_model_rollout  persistent learned-model rollout (sampling.py:16-89, trajectory_rollout :96-123 with the policy stage off):
//                    a workgroup owns a tile of DYN_RT trajectories of one member and walks all H steps itself:
//                    policy forward (tanh FCNetwork with its transforms) -> + noise * exp(log_std) -> clamp -> dynamics -> clamp
//   k_dyn_prep       normalised inputs and regression targets, once per fit (nn_dynamics.py:98-110, 134-147)
//   k_dyn_fit        persistent single-workgroup minibatch-Adam trainer (fit_model, nn_dynamics.py:344-385)
//   k_dl_*           the launch-based route of the same fit, for shapes whose minibatch does not fit in LDS
//   k_dyn_pred_err   ensemble-disagreement truncation (model_accel_npg.py:137-155)
//
// Parameters use torch's layout: per member one flat vector [W1 (h1 x d_in) row-major, b1, ..., W_out, b_out] (the order of
// DynamicsNet.parameters()); transforms per member [in_shift (d_in), in_scale (d_in), out_shift (d_out), out_scale (d_out)] over
// the CONCATENATED input ([s, a] or [s, a, s']; the host repeats RewardNet's s transforms for s').
//
// Rollout LDS budget (per workgroup, fp32): the whole policy (P_pol floats: 17 k = 68 KiB for 64 x 64 at n = 200 inputs) +
// the tile's [s, a] (DYN_RT x (n + m)) + four DYN_RT x W activation blocks (W = widest layer of either net; 4 x 8 x 256 x 4 B =
// 32 KiB at 256).  DYN_RT = 8 trajectories per workgroup: K = 4 members x N = 250 paths = 128 workgroups, about one per CU
// pair, and every weight a thread reads serves DYN_RPG = 4 rows.  The dynamics net is NOT in LDS: a 256-wide net's W2 alone is
// 256 KiB in fp32 against 160 KiB per CU; its weights stream from L2 (4 MiB per XCD) every step -- all workgroups of a member
// read the same lines.
//
// Fit LDS budget (k_dyn_fit, 1024 threads, weights and Adam moments in global memory / L2, every one owned by one thread for
// the update): the minibatch's activations of every layer, its targets and two delta blocks, B x (d_in + sum(h) + 2 d_out +
// 2 max(h, d_out)) floats -- (64, 64) at d_in 30, d_out 20, B 64: 64 KiB.  Shapes up to hidden 128 and batch 64 take this route
// while that budget plus the kernel's 128 B of static LDS fits in 160 KiB; the rest (256 x 256, RewardNet's 100 x 100 at large
// inputs) run k_dl_*: per Adam step one gather, one launch per layer forward, a loss head, one backward launch per hidden layer
// and one gradient + Adam launch per layer, activations in a global scratch block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vecops.h"

namespace mjx {

enum { DYN_ACT_RELU = 0, DYN_ACT_TANH = 1 };
enum { DYN_OUT_AFFINE = 1, DYN_MASK = 2, DYN_RESIDUAL = 4 };
// fit targets: loss through the output affine on raw y (RewardNet, fit_reward keeps the out transforms on), or transformed
// targets (y - out_shift) / (out_scale + 1e-8), or residual targets (y - s - out_shift) / (out_scale + 1e-8) with s = x[:, :d_out]
enum { DYN_TGT_AFFINE = 0, DYN_TGT_PLAIN = 1, DYN_TGT_RESIDUAL = 2 };
constexpr int DYN_MAXL = 8;           // Linear layers per net (hidden + output)
constexpr int DYN_RT = 8;             // rollout: trajectories per workgroup
constexpr int DYN_FT = 32;            // forward: rows per workgroup
constexpr int DYN_RPG = 4;            // rows per thread in a layer product
__host__ __device__ constexpr int pad8(int d) { return (d + 7) & ~7; }   // a layer's K dimension in whole groups of eight (the MFMA kernels)

struct DynNet {
  int nl = 0;                         // Linear layers
  int sz[DYN_MAXL + 1] = {};          // d_in, h..., d_out
  int64_t oW[DYN_MAXL] = {}, ob[DYN_MAXL] = {};
  int64_t P = 0;
  int maxw = 0;                       // widest layer, inputs included
  __host__ bool init(const int* sizes, int n) {
    if (n < 2 || n > DYN_MAXL + 1) return false;
    nl = n - 1; P = 0; maxw = 0;
    for (int i = 0; i < n; ++i) { if (sizes[i] <= 0) return false; sz[i] = sizes[i]; maxw = sizes[i] > maxw ? sizes[i] : maxw; }
    for (int l = 0; l < nl; ++l) { oW[l] = P; P += (int64_t)sz[l] * sz[l + 1]; ob[l] = P; P += sz[l + 1]; }
    return true;
  }
  __host__ __device__ int din() const { return sz[0]; }
  __host__ __device__ int dout() const { return sz[nl]; }
};

__device__ __forceinline__ float dyn_act(float x, int act) { return act == DYN_ACT_TANH ? tanhf(x) : fmaxf(x, 0.f); }
// derivative from the layer's OUTPUT (torch's relu / tanh backward: grad * (y > 0), grad * (1 - y^2))
__device__ __forceinline__ float dyn_dact(float y, int act) { return act == DYN_ACT_TANH ? 1.f - y * y : (y > 0.f ? 1.f : 0.f); }
// a dynamics net's raw output z of unit i under the output flags: affine (out_scale + 1e-8, out_shift), the mask of the units whose
// out_scale is below 1e-8, the residual resid() -- each read only where its flag is set
template <class Resid>
__device__ __forceinline__ float dyn_out_flags(float z, int flags, const float* osh, const float* osc, int i, Resid resid) {
  if (flags & DYN_OUT_AFFINE) z = z * (osc[i] + 1e-8f) + osh[i];
  if (flags & DYN_MASK) z = z * (osc[i] >= 1e-8f ? 1.f : 0.f);
  if (flags & DYN_RESIDUAL) z = z + resid();
  return z;
}

// out[r][j] = act(b[j] + sum_i in[r][i] W[j][i]) for r < rows, j < dout (act < 0: none).  in / out row strides ldi / ldo; W, b in
// torch layout, in global memory or LDS.  A thread owns one unit j and DYN_RPG rows: every weight it loads serves DYN_RPG rows,
// and the lanes of a wave (consecutive j, same rows) read the same activation words (LDS broadcast).
__device__ void dyn_dense(const float* in, int ldi, int rows, int din, const float* __restrict__ W, const float* __restrict__ b,
                          int dout, float* out, int ldo, int act) {
  const int ng = (rows + DYN_RPG - 1) / DYN_RPG;
  for (int idx = threadIdx.x; idx < dout * ng; idx += blockDim.x) {
    const int j = idx % dout, r0 = (idx / dout) * DYN_RPG;
    const float* ip[DYN_RPG];
#pragma unroll
    for (int q = 0; q < DYN_RPG; ++q) ip[q] = in + (int64_t)(r0 + q < rows ? r0 + q : rows - 1) * ldi;
    float acc[DYN_RPG];
#pragma unroll
    for (int q = 0; q < DYN_RPG; ++q) acc[q] = 0.f;
    const float* w = W + (int64_t)j * din;
    for (int i = 0; i < din; ++i) {
      const float wi = w[i];
#pragma unroll
      for (int q = 0; q < DYN_RPG; ++q) acc[q] = fmaf(ip[q][i], wi, acc[q]);
    }
    const float bj = b[j];
#pragma unroll
    for (int q = 0; q < DYN_RPG; ++q)
      if (r0 + q < rows) { const float z = acc[q] + bj; out[(int64_t)(r0 + q) * ldo + j] = act < 0 ? z : dyn_act(z, act); }
  }
}

// one net over a tile of rows: x (rows x d_in, raw, row stride ldx) -> y (rows x d_out, row stride ldy).
// xn, b0, b1: LDS blocks of rows x maxw.  Ends with a barrier (y is complete and x may be overwritten).
__device__ void dyn_net_tile(const DynNet& net, const float* __restrict__ P, const float* __restrict__ tr, int act, int flags,
                             const float* x, int ldx, int rows, float* xn, float* b0, float* b1, float* y, int ldy) {
  const int din = net.din(), dout = net.dout(), W = net.maxw;
  for (int e = threadIdx.x; e < rows * din; e += blockDim.x) {
    const int r = e / din, i = e - r * din;
    xn[r * W + i] = (x[(int64_t)r * ldx + i] - tr[i]) / (tr[din + i] + 1e-8f);
  }
  __syncthreads();
  const float* in = xn;
  float* bufs[2] = {b0, b1};
  for (int l = 0; l < net.nl; ++l) {
    float* o = bufs[l & 1];
    dyn_dense(in, W, rows, net.sz[l], P + net.oW[l], P + net.ob[l], net.sz[l + 1], o, W, l + 1 < net.nl ? act : -1);
    __syncthreads();
    in = o;
  }
  const float* osh = tr + 2 * din;
  const float* osc = osh + dout;
  for (int e = threadIdx.x; e < rows * dout; e += blockDim.x) {
    const int r = e / dout, j = e - r * dout;
    y[(int64_t)r * ldy + j] = dyn_out_flags(in[r * W + j], flags, osh, osc, j, [&] { return x[(int64_t)r * ldx + j]; });
  }
  __syncthreads();
}

// ---- (a) batched forward: grid (ceil(rows / DYN_FT), K), 256 threads
struct DynFwdArgs {
  DynNet net;
  const float* x; int64_t x_stride;   // member k reads x + k * x_stride (0: all members see the same rows)
  int64_t rows;
  const float* P; const float* tr;    // K x P, K x (2 d_in + 2 d_out)
  int act, flags;
  float* out;                         // K x rows x d_out
};

__global__ __launch_bounds__(256) void k_dyn_forward(DynFwdArgs a) {
  extern __shared__ float dfs[];
  const int W = a.net.maxw;
  float* xn = dfs; float* b0 = xn + DYN_FT * W; float* b1 = b0 + DYN_FT * W;
  const int k = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * DYN_FT;
  const int rows = (int)(a.rows - r0 < DYN_FT ? a.rows - r0 : DYN_FT);
  const int din = a.net.din(), dout = a.net.dout();
  dyn_net_tile(a.net, a.P + k * a.net.P, a.tr + (int64_t)k * (2 * din + 2 * dout), a.act, a.flags,
               a.x + k * a.x_stride + r0 * din, din, rows, xn, b0, b1, a.out + ((int64_t)k * a.rows + r0) * dout, dout);
}

// ---- (b) persistent learned-model rollout: grid (ceil(N / DYN_RT), K), 256 threads
struct RolloutArgs {
  int64_t N; int H;
  const float* s0;                    // N x n
  const float* actions;               // N x H x m (trajectory_rollout; policy stage off) or null
  DynNet pol; const float* pol_P;     // tanh FCNetwork, flat [W, b, ..., log_std (m)]
  const float* pol_tr;                // [in_shift n, in_scale n, out_shift m, out_scale m]
  const float* noise;                 // K x H x N x m standard normals, or null (eval_mode)
  DynNet dyn; const float* dyn_P; const float* dyn_tr; int act, flags;
  const float* a_lo; const float* a_hi; const float* s_lo; const float* s_hi;   // fp32 bounds (m / n); null: no clamp
  float* obs;                         // K x N x H x n   (the state BEFORE step t)
  float* act_out;                     // K x N x H x m
  int W;                              // widest layer of either net
};

// torch.max(torch.min(x, hi), lo) (sampling.py:315), NaN passes through as in torch
__device__ __forceinline__ float dyn_clamp(float x, float lo, float hi) { x = x > hi ? hi : x; return x < lo ? lo : x; }

__global__ __launch_bounds__(256) void k_model_rollout(RolloutArgs a) {
  extern __shared__ float rls[];
  const bool use_pol = a.actions == nullptr;
  const int n = a.dyn.dout(), m = a.dyn.din() - n, nm = n + m, W = a.W;
  const int64_t Ppol = use_pol ? a.pol.P + m : 0;
  float* polw = rls;                                  // the whole policy (+ log_std), loaded once
  float* sa = polw + ((Ppol + 3) & ~3);               // DYN_RT x (n + m): [s, a] of the tile
  float* xn = sa + DYN_RT * nm;
  float* b0 = xn + DYN_RT * W;
  float* b1 = b0 + DYN_RT * W;
  float* y = b1 + DYN_RT * W;
  const int tid = threadIdx.x, k = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * DYN_RT;
  const int rows = (int)(a.N - i0 < DYN_RT ? a.N - i0 : DYN_RT);
  for (int64_t e = tid; e < Ppol; e += blockDim.x) polw[e] = a.pol_P[e];
  for (int e = tid; e < rows * n; e += blockDim.x) { const int r = e / n, j = e - r * n; sa[r * nm + j] = a.s0[(i0 + r) * n + j]; }
  __syncthreads();
  const float* dP = a.dyn_P + k * a.dyn.P;
  const float* dtr = a.dyn_tr + (int64_t)k * (2 * a.dyn.din() + 2 * n);
  for (int t = 0; t < a.H; ++t) {
    if (use_pol) {
      // policy mean: (s - in_shift) / (in_scale + 1e-8) -> tanh layers -> out * out_scale + out_shift (fc_network.py:39-52)
      const float* ptr_ = a.pol_tr;
      for (int e = tid; e < rows * n; e += blockDim.x) {
        const int r = e / n, i = e - r * n;
        xn[r * W + i] = (sa[r * nm + i] - ptr_[i]) / (ptr_[n + i] + 1e-8f);
      }
      __syncthreads();
      const float* in = xn;
      float* bufs[2] = {b0, b1};
      for (int l = 0; l < a.pol.nl; ++l) {
        float* o = bufs[l & 1];
        dyn_dense(in, W, rows, a.pol.sz[l], polw + a.pol.oW[l], polw + a.pol.ob[l], a.pol.sz[l + 1], o, W,
                  l + 1 < a.pol.nl ? DYN_ACT_TANH : -1);
        __syncthreads();
        in = o;
      }
      const float* ls = polw + a.pol.P;
      for (int e = tid; e < rows * m; e += blockDim.x) {
        const int r = e / m, j = e - r * m;
        float v = in[r * W + j] * ptr_[2 * n + m + j] + ptr_[2 * n + j];
        if (a.noise) v = v + a.noise[(((int64_t)k * a.H + t) * a.N + i0 + r) * m + j] * expf(ls[j]);
        if (a.a_lo) v = dyn_clamp(v, a.a_lo[j], a.a_hi[j]);
        sa[r * nm + n + j] = v;
      }
    } else {
      for (int e = tid; e < rows * m; e += blockDim.x) {
        const int r = e / m, j = e - r * m;
        float v = a.actions[((i0 + r) * a.H + t) * m + j];
        if (a.a_lo) v = dyn_clamp(v, a.a_lo[j], a.a_hi[j]);
        sa[r * nm + n + j] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < rows * nm; e += blockDim.x) {
      const int r = e / nm, j = e - r * nm;
      const int64_t row = ((int64_t)k * a.N + i0 + r) * a.H + t;
      if (j < n) a.obs[row * n + j] = sa[r * nm + j];
      else a.act_out[row * m + (j - n)] = sa[r * nm + j];
    }
    dyn_net_tile(a.dyn, dP, dtr, a.act, a.flags, sa, nm, rows, xn, b0, b1, y, n);
    for (int e = tid; e < rows * n; e += blockDim.x) {
      const int r = e / n, j = e - r * n;
      float v = y[r * n + j];
      if (a.s_lo) v = dyn_clamp(v, a.s_lo[j], a.s_hi[j]);
      sa[r * nm + j] = v;
    }
    __syncthreads();
  }
}

// ---- (c) fit: prep (normalised inputs, targets), then Adam steps
__global__ void k_dyn_prep(const float* __restrict__ x, const float* __restrict__ y, int64_t N, int din, int dout,
                           const float* __restrict__ in_tr, const float* __restrict__ out_tr, int tmode,
                           float* __restrict__ xn, float* __restrict__ tg) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N * din; e += stride) {
    const int i = (int)(e % din);
    xn[e] = (x[e] - in_tr[i]) / (in_tr[din + i] + 1e-8f);
  }
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N * dout; e += stride) {
    const int64_t r = e / dout; const int j = (int)(e - r * dout);
    float v = y[e];
    if (tmode == DYN_TGT_RESIDUAL) v = ((v - x[r * din + j]) - out_tr[j]) / (out_tr[dout + j] + 1e-8f);
    else if (tmode == DYN_TGT_PLAIN) v = (v - out_tr[j]) / (out_tr[dout + j] + 1e-8f);
    tg[e] = v;
  }
}

struct DynFitArgs {
  DynNet net;
  const float* xn; const float* tg;   // N x d_in normalised inputs, N x d_out targets (k_dyn_prep)
  const int32_t* idx;                 // steps x B row indices (the first (N // B) x B entries of each epoch's permutation)
  int64_t steps; int B;
  float* P; float* m; float* v;       // flat parameters and Adam moments (global, updated in place)
  int64_t step0;                      // Adam steps taken before this call
  float lr, wd;
  int act;
  const float* out_tr;                // DYN_TGT_AFFINE: [out_shift, out_scale] (the loss runs through the output affine), else null
  float* loss;                        // per step: the minibatch MSE
};

// torch.optim.Adam (amsgrad off, L2 weight decay folded into the gradient, bias-corrected, eps 1e-8), as k_adam in baseline.h,
// exact divides, the fp32-beta constants (vecops.h)
__device__ __forceinline__ void dyn_adam(float* p, float* m, float* v, int64_t i, float g, float lr_bc1, float bc2s, float wd) {
  const float pi = p[i];
  const float gi = g + wd * pi;
  const float mi = m[i] + (gi - m[i]) * ADAM32_C1;
  const float vi = v[i] * ADAM32_B2 + gi * gi * ADAM32_C2;
  m[i] = mi; v[i] = vi;
  const float denom = sqrtf(vi) / bc2s + ADAM_EPS;
  p[i] = pi - lr_bc1 * (mi / denom);
}
__device__ __forceinline__ void dyn_bias_corr(int64_t t, float lr, float& lr_bc1, float& bc2s) {
  lr_bc1 = (float)((double)lr / (1.0 - pow(0.9, (double)t)));
  bc2s = (float)sqrt(1.0 - pow(0.999, (double)t));
}

// loss head on the output block z (B x d_out, row stride ldz): delta = dMSE/dz, returns this thread's share of sum(err^2)
__device__ __forceinline__ double dyn_loss_head(const float* z, int ldz, const float* tg, int B, int dout, const float* out_tr,
                                                float* delta, int ldd, int e) {
  const int r = e / dout, j = e - r * dout;
  float yv = z[r * ldz + j], s = 1.f;
  if (out_tr) { s = out_tr[dout + j] + 1e-8f; yv = yv * s + out_tr[j]; }
  const float err = yv - tg[r * dout + j];
  delta[r * ldd + j] = (2.0f / (float)(B * dout)) * err * s;
  return (double)err * (double)err;
}

// persistent route: ONE workgroup of 1024 threads runs every step
__global__ __launch_bounds__(1024) void k_dyn_fit(DynFitArgs a) {
  extern __shared__ float fls[];
  __shared__ double red[16];
  const DynNet& net = a.net;
  const int B = a.B, nl = net.nl, din = net.din(), dout = net.dout(), tid = threadIdx.x;
  int wmax = 0; for (int l = 1; l <= nl; ++l) wmax = net.sz[l] > wmax ? net.sz[l] : wmax;
  float* A[DYN_MAXL + 1];                             // A[0] = inputs, A[l] = output of layer l (B x sz[l], dense rows)
  float* q = fls;
  for (int l = 0; l <= nl; ++l) { A[l] = q; q += B * net.sz[l]; }
  float* T = q; q += B * dout;
  float* D0 = q; q += B * wmax;
  float* D1 = q;
  for (int64_t s = 0; s < a.steps; ++s) {
    const int32_t* ix = a.idx + s * B;
    for (int e = tid; e < B * din; e += blockDim.x) { const int r = e / din, i = e - r * din; A[0][e] = a.xn[(int64_t)ix[r] * din + i]; }
    for (int e = tid; e < B * dout; e += blockDim.x) { const int r = e / dout, j = e - r * dout; T[e] = a.tg[(int64_t)ix[r] * dout + j]; }
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      dyn_dense(A[l], net.sz[l], B, net.sz[l], a.P + net.oW[l], a.P + net.ob[l], net.sz[l + 1], A[l + 1], net.sz[l + 1],
                l + 1 < nl ? a.act : -1);
      __syncthreads();
    }
    double part = 0.0;
    for (int e = tid; e < B * dout; e += blockDim.x) part += dyn_loss_head(A[nl], dout, T, B, dout, a.out_tr, D0, dout, e);
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += red[w];
      a.loss[s] = (float)(tot / (double)(B * dout));
    }
    float lr_bc1, bc2s;
    dyn_bias_corr(a.step0 + s + 1, a.lr, lr_bc1, bc2s);
    float* dz = D0; float* dn = D1;
    for (int l = nl - 1; l >= 0; --l) {
      const int di = net.sz[l], dj = net.sz[l + 1];
      const float* Wl = a.P + net.oW[l];
      if (l > 0) {                                    // delta of layer l's input, with W_l before its update
        for (int e = tid; e < B * di; e += blockDim.x) {
          const int r = e / di, i = e - r * di;
          float g = 0.f;
          for (int j = 0; j < dj; ++j) g = fmaf(dz[r * dj + j], Wl[(int64_t)j * di + i], g);
          dn[e] = g * dyn_dact(A[l][e], a.act);
        }
        __syncthreads();
      }
      const int nw = di * dj;
      for (int e = tid; e < nw + dj; e += blockDim.x) {
        float g = 0.f;
        if (e < nw) { const int j = e / di, i = e - j * di; for (int r = 0; r < B; ++r) g = fmaf(dz[r * dj + j], A[l][r * di + i], g); }
        else { const int j = e - nw; for (int r = 0; r < B; ++r) g += dz[r * dj + j]; }
        dyn_adam(a.P, a.m, a.v, net.oW[l] + e, g, lr_bc1, bc2s, a.wd);
      }
      __syncthreads();
      float* t_ = dz; dz = dn; dn = t_;
    }
  }
}

// launch-based route: one thread per output element
__global__ void k_dl_gather(const float* __restrict__ xn, const float* __restrict__ tg, const int32_t* __restrict__ ix, int B, int din,
                            int dout, float* __restrict__ X, float* __restrict__ T) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B * (din + dout); e += gridDim.x * blockDim.x) {
    if (e < B * din) { const int r = e / din, i = e - r * din; X[e] = xn[(int64_t)ix[r] * din + i]; }
    else { const int f = e - B * din, r = f / dout, j = f - r * dout; T[f] = tg[(int64_t)ix[r] * dout + j]; }
  }
}
__global__ void k_dl_fwd(const float* __restrict__ in, int B, int di, const float* __restrict__ Wl, const float* __restrict__ bl, int dj,
                         float* __restrict__ out, int act) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B * dj; e += gridDim.x * blockDim.x) {
    const int r = e / dj, j = e - r * dj;
    float g = 0.f;
    for (int i = 0; i < di; ++i) g = fmaf(in[r * di + i], Wl[(int64_t)j * di + i], g);
    const float z = g + bl[j];
    out[e] = act < 0 ? z : dyn_act(z, act);
  }
}
__global__ __launch_bounds__(1024) void k_dl_loss(const float* __restrict__ z, const float* __restrict__ T, int B, int dout,
                                                  const float* __restrict__ out_tr, float* __restrict__ delta, float* __restrict__ loss) {
  __shared__ double red[16];
  double part = 0.0;
  for (int e = threadIdx.x; e < B * dout; e += blockDim.x) part += dyn_loss_head(z, dout, T, B, dout, out_tr, delta, dout, e);
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += red[w];
    loss[0] = (float)(tot / (double)(B * dout));
  }
}
__global__ void k_dl_bwd(const float* __restrict__ dz, int B, int di, const float* __restrict__ Wl, int dj, const float* __restrict__ Al,
                         int act, float* __restrict__ dn) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B * di; e += gridDim.x * blockDim.x) {
    const int r = e / di, i = e - r * di;
    float g = 0.f;
    for (int j = 0; j < dj; ++j) g = fmaf(dz[r * dj + j], Wl[(int64_t)j * di + i], g);
    dn[e] = g * dyn_dact(Al[e], act);
  }
}
__global__ void k_dl_adam(const float* __restrict__ dz, const float* __restrict__ Al, int B, int di, int dj, float* P, float* m, float* v,
                          int64_t off, int64_t t, float lr, float wd) {
  float lr_bc1, bc2s;
  dyn_bias_corr(t, lr, lr_bc1, bc2s);
  const int nw = di * dj;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nw + dj; e += gridDim.x * blockDim.x) {
    float g = 0.f;
    if (e < nw) { const int j = e / di, i = e - j * di; for (int r = 0; r < B; ++r) g = fmaf(dz[r * dj + j], Al[r * di + i], g); }
    else { const int j = e - nw; for (int r = 0; r < B; ++r) g += dz[r * dj + j]; }
    dyn_adam(P, m, v, off + e, g, lr_bc1, bc2s, wd);
  }
}

// ---- (d) truncation: err[r] = max_k mean_j (s_next[r][j] - pred[k][r][j])^2 over the rows of segment g = [off[g], off[g+1]);
// first[g] = index (within the segment) of the first row with err > lim, -1 if none.  One workgroup per segment.  As the
// reference's np.maximum, a row where any member's error is NaN has a NaN error, and NaN > lim is false.
__global__ __launch_bounds__(256) void k_dyn_pred_err(const float* __restrict__ pred, int K, int64_t rows, int n,
                                                      const float* __restrict__ s_next, const int64_t* __restrict__ off, double lim,
                                                      float* __restrict__ err, int32_t* __restrict__ first) {
  __shared__ int64_t hit;
  const int g = blockIdx.x;
  const int64_t a0 = off[g], a1 = off[g + 1];
  if (threadIdx.x == 0) hit = a1;
  __syncthreads();
  for (int64_t r = a0 + threadIdx.x; r < a1; r += blockDim.x) {
    float e = 0.f;
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) { const float d = s_next[r * n + j] - pred[((int64_t)k * rows + r) * n + j]; s += (double)(d * d); }
      const float mk = (float)(s / n);
      if (k == 0 || mk > e || mk != mk) e = mk;       // np.maximum: a NaN member makes the row NaN (fmaxf would drop it)
    }
    err[r] = e;
    if ((double)e > lim) atomicMin((unsigned long long*)&hit, (unsigned long long)r);
  }
  __syncthreads();
  if (threadIdx.x == 0) first[g] = hit < a1 ? (int32_t)(hit - a0) : -1;
}

}  // namespace mjx
