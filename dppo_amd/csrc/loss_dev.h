// The policy half of the PPO loss for a 64-sample tile whose inputs are already in LDS (fused_forward_merged_loss_kernel's epilogue:
// the forward's own output tile, the gathered chain pair, old log-probs and advantage), in the three phases the epilogue spreads
// over the workgroup: per (sample, element) the clamped log-probs and the gradient source, per sample the two sums and the row
// math, per (sample, 16-byte chunk) the d loss / d eps row.  The arithmetic is ppo_loss_kernel's (ppo.hip, NREG = 16), statement
// by statement: log-probs summed over j in ascending order from 0.f, the same clamp / ratio / clip-schedule / surrogate
// expressions, the same d loss / d eps.  fused.hip is compiled with floating-point contraction ON (its Mish must round as the
// inference forward's does); everything here must round as ppo.hip's kernels do (-ffp-contract=off) or the recomputed log-probs
// stop matching the precomputed ones bit for bit -- hence the pragma in every function body, and a private copy of the posterior
// (posterior.h belongs to the contraction-off translation units).
#pragma once
#include "common.h"
#include "dppo_hip.h"
#include "ppo.h"

namespace dppo {

#ifndef DPPO_LOG_SQRT_2PI
#define DPPO_LOG_SQRT_2PI 0.91893853320467274178f
#endif

// VPGDiffusion.p_mean_var (diffusion_vpg.py:165-223) and its derivative wrt eps: posterior.h's function, contraction off
__device__ __forceinline__ void posterior_nc(const dppo_diffusion_cfg& c, const dppo_step& st, float x, float eps, float& mu,
                                             float& dmu_deps) {
#pragma clang fp contract(off)
  if (!c.use_ddim) {
    float x0 = st.c0 * x - st.c1 * eps;
    float pass = 1.f;
    if (c.has_denoised_clip) {
      pass = (x0 >= -c.denoised_clip && x0 <= c.denoised_clip) ? 1.f : 0.f;
      x0 = fminf(fmaxf(x0, -c.denoised_clip), c.denoised_clip);
    }
    mu = st.c2 * x0 + st.c3 * x;
    dmu_deps = -(st.c2 * st.c1) * pass;
  } else {
    float x0 = (x - st.c1 * eps) / st.c0;
    float dx0 = -st.c1 / st.c0;
    float e2 = eps, de2 = 1.f;
    if (c.has_denoised_clip) {
      const float pass = (x0 >= -c.denoised_clip && x0 <= c.denoised_clip) ? 1.f : 0.f;
      x0 = fminf(fmaxf(x0, -c.denoised_clip), c.denoised_clip);
      dx0 *= pass;
      e2 = (x - st.c0 * x0) / st.c1;
      de2 = -(st.c0 / st.c1) * dx0;
    }
    if (c.has_eps_clip) {
      const float pass = (e2 >= -c.eps_clip && e2 <= c.eps_clip) ? 1.f : 0.f;
      e2 = fminf(fmaxf(e2, -c.eps_clip), c.eps_clip);
      de2 *= pass;
    }
    mu = st.c2 * x0 + st.c3 * e2;
    dmu_deps = st.c2 * dx0 + st.c3 * de2;
  }
}

// LDS rows of the three per-element arrays: 17 dwords, so that the sample phase's lanes (one row each) hit 64 different banks
constexpr int LOSS_ROW = 17;
// a denoising step as the prologue stages it in LDS: c0, c1, c2, c3, std, log std (the row builder's), two dwords of padding
constexpr int LOSS_STEP = 8;

// Element phase: one (sample, element) pair -- ppo_loss_kernel's `element` without its two adds.  step: the sample's LOSS_STEP
// dwords.  lpn / lpo: the clamped new / old log-prob, gs: (d / var) d mu / d eps where the clamp passes the gradient, else 0.
__device__ __forceinline__ void loss_element_nc(const dppo_diffusion_cfg& dc, const float* step, float x, float xn, float e, float o,
                                                float& lpn, float& lpo, float& gs) {
#pragma clang fp contract(off)
  dppo_step st;
  st.c0 = lds_load(step), st.c1 = lds_load(step + 1), st.c2 = lds_load(step + 2), st.c3 = lds_load(step + 3);
  st.std = lds_load(step + 4);
  // (log std_k from the table: logf expands differently under this translation unit's contraction setting, pragma or not)
  const float var = st.std * st.std, lstd = lds_load(step + 5);
  float mu, dmu;
  posterior_nc(dc, st, x, e, mu, dmu);
  const float d = xn - mu;
  const float lp = -(d * d) / (2.f * var) - lstd - DPPO_LOG_SQRT_2PI;
  lpn = fminf(fmaxf(lp, -5.f), 2.f);
  lpo = fminf(fmaxf(o, -5.f), 2.f);
  gs = (lp >= -5.f && lp <= 2.f) ? (d / var) * dmu : 0.f;
}

// Sample phase: the two sums over the sample's clamped log-probs (LDS rows lpn / lpo, cnt elements, j ascending from 0.f: the
// loss kernel's adds in the loss kernel's order) and the row math.  tab: [Kft] denoising discount, [Kft] clip range, adv mean,
// adv std, the (global) minibatch's sample count as a float.  Returns coef = d mean(L) / d lp_j (before the clamp mask); s4: pg
// loss, approx kl, clip fraction, ratio.
__device__ __forceinline__ float policy_loss_sample_nc(const dppo_ppo_cfg& pc, const float* tab, int k, float adv, const float* lpn,
                                                       const float* lpo, int cnt, double (&s4)[4]) {
#pragma clang fp contract(off)
  const int Kft = pc.ft_denoising_steps;
  // (all sixteen slots of both rows are read at once -- a row has LOSS_ROW of them -- and only the adds are serial)
  float vn[16], vo[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) vn[j] = lds_load(lpn + j), vo[j] = lds_load(lpo + j);
  float sum_new = 0.f, sum_old = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < cnt) {
      sum_new += vn[j];
      sum_old += vo[j];
    }
  }
  const float newlp = sum_new / (float)cnt, oldlp = sum_old / (float)cnt;
  if (pc.norm_adv) adv = (adv - lds_load(tab + 2 * Kft)) / (lds_load(tab + 2 * Kft + 1) + 1e-8f);
  if (pc.has_adv_clip) adv = fminf(fmaxf(adv, pc.adv_clip_lo), pc.adv_clip_hi);
  adv *= lds_load(tab + k);
  const float logratio = newlp - oldlp;
  const float ratio = expf(logratio);
  const float eps_k = lds_load(tab + Kft + k);
  const float lo = 1.f - eps_k, hi = 1.f + eps_k;
  const float rc = fminf(fmaxf(ratio, lo), hi);
  const float pg1 = -adv * ratio, pg2 = -adv * rc;
  const float w1 = pg1 > pg2 ? 1.f : (pg1 == pg2 ? 0.5f : 0.f);
  const float within = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
  const float dL_dratio = -adv * (w1 + (1.f - w1) * within);
  const float coef = dL_dratio * ratio / (lds_load(tab + 2 * Kft + 2) * (float)cnt);
  s4[0] = fmaxf(pg1, pg2);
  s4[1] = (double)((ratio - 1.f) - logratio);
  s4[2] = fabsf(ratio - 1.f) > eps_k ? 1.0 : 0.0;
  s4[3] = ratio;
  return coef;
}

// Store phase: 16-byte chunk c of a sample's d loss / d eps row (bf16, eight elements: ppo_loss_kernel's pack_store): coef * gs for
// the elements below cnt (gs is 0.f where the clamp did not pass: the product, not a constant, as there), zero padding behind.
__device__ __forceinline__ u32x4 policy_loss_chunk_nc(float coef, const float* gs, int c, int cnt) {
#pragma clang fp contract(off)
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = c * 8 + q < cnt ? coef * lds_load(gs + c * 8 + q) : 0.f;
  u32x4 w;
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = (uint32_t)f2bf(v[2 * q]) | ((uint32_t)f2bf(v[2 * q + 1]) << 16);
  return w;
}

}  // namespace dppo
