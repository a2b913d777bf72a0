// Soft actor-critic (SAC): the reference's SAC_Gaussian.loss_critic / loss_actor / loss_temperature (model/rl/gaussian_sac.py:31-80)
// and GaussianModel.forward's get_logprob / reparameterize / tanh_output branches (model/common/gaussian.py:85-120) on a
// Gaussian_MLP with the state-dependent logvar head (model/common/mlp_gaussian.py:304-321, 370-379), around the plain-MLP forward /
// backward every other path uses.  To the library the actor is a kind-1 plain trunk with out_dim = 2 AF whose output row is
// [mean | raw logvar].  New here: the two-headed epilogue (sample, squash, log-probability) and its backward, the per-row choice of
// the twin in the critic's data-gradient chain (qsm.h) and the entropy terms of the TD target and of the temperature loss.
//
// Launches per call on the shipped shape (two hidden layers: n_blocks = 1), side-stream events aside:
//   dppo_sac_sample          1 row builder + 3 GEMMs + 1 head epilogue                                                  =  5
//   dppo_sac_q_loss_fwd_bwd  1 row builder + 4 x 3 GEMMs (side by side) + 2 loss + the twin's two parameter backwards
//   dppo_sac_actor_fwd_bwd   1 row builder + 3 GEMMs (actor) + 1 head epilogue + 2 x 3 GEMMs (Q1 | Q2) + 1 W0 pack + 1 select/seed
//                            + 2 x 1 chain GEMM + 1 tail/head backward + 1 statistics                                  = 17
//                            (bf16: + 2 for the heads' bias gradient from the unrounded d_out)
//                            + the actor's parameter backward; nothing of the critic's (no weight gradient, column sum or buffer)
//   dppo_sac_alpha_loss      1
// None of them reads the device on the host: alpha and log_alpha are device scalars.
#pragma once
#include "qsm.h"

namespace dppo {

constexpr int SAC_RPB = 16;  // rows per 256-thread block of the head epilogue (16 lanes per row)

// One element of the head, forward.  With c = 0.5 (lmax - lmin):  lv = lmin + c (tanh(raw) + 1);  sigma = exp(0.5 lv) (1e-4 when
// deterministic);  zc = clamp(z, +-randn_clip);  u = mu + sigma zc;  a = tanh(u), s = 1 - a^2 (squash) or a = u, s = 1.
// s and 1 - tanh(raw)^2 are formed as 4 e / (1 + e)^2 with e = exp(-2 |x|): 1 - tanhf(x)^2 is 0 in fp32 from |x| ~ 9.
struct SacHead {
  dppo_sac_cfg cfg;
  float half_span;  // 0.5f * (logvar_max - logvar_min), rounded to fp32 once like the reference's tensor arithmetic
  IdqlRows ring;    // where obs comes from (actor call: the critic rows are built from it); N, OD, AD = AF
  const float* out;  // [N][ldo] trunk output: columns [0, AF) mean, [AF, 2 AF) raw logvar
  int ldo, AF;
  const float* noise;  // [N][AF] or null: Philox keyed by cfg.seed_lo / seed_hi, counter = element index
  float *actions, *u_out, *logp;  // [N][AF], [N][AF], [N]: any may be null
  float* sig_row;                 // [N] sum over AF of sigma, or null
  void *q1in, *q2in;              // [N][KpQ] elem [obs | a | 0], or null (sampling)
  int KpQ;
};
template <class P>
void launch_sac_head(const SacHead& a, hipStream_t s);

// (shared by sac.hip and rlpd.hip: RLPD's actor head is this one)
#define SAC_LOG_SQRT_2PI 0.91893853320467274178f

// ---- the head, element by element -------------------------------------------------------------------------------------------
// 1 - tanh(x)^2 without the cancellation
__device__ __forceinline__ float sac_sech2(float x) {
  const float e = expf(-2.f * fabsf(x));
  const float d = 1.f + e;
  return (4.f * e) / (d * d);
}
struct SacElem {
  float zc, lv, sigma, u, a, s, raw;
};
__device__ __forceinline__ SacElem sac_elem(const SacHead& a, int64_t n, int j) {
  const dppo_sac_cfg& c = a.cfg;
  SacElem e;
  const float mu = a.out[n * a.ldo + j];
  e.raw = a.out[n * a.ldo + a.AF + j];
  const int64_t i = n * a.AF + j;
  const float z = a.noise != nullptr ? a.noise[i] : philox_normal((uint64_t)i, c.seed_lo, c.seed_hi);
  e.zc = fminf(fmaxf(z, -c.randn_clip), c.randn_clip);
  const float t1 = tanhf(e.raw) + 1.f;
  const float t2 = a.half_span * t1;
  e.lv = c.logvar_min + t2;
  e.sigma = c.deterministic ? 1e-4f : expf(0.5f * e.lv);
  const float p = e.sigma * e.zc;
  e.u = mu + p;
  if (c.squash) {
    e.a = tanhf(e.u);
    e.s = sac_sech2(e.u);
  } else {
    e.a = e.u;
    e.s = 1.f;
  }
  return e;
}

// sel[n] = q2 < q1 (ties go to q1, like the first argument of torch.min);  qsel[n] = the smaller;  and the seed of both trunks'
// data-gradient chains: dz_i[n][h] = elem(wout_i[h] * act'(z_i[n][h])) for the selected trunk i of row n, 0 for the other
struct SacSelect {
  const float *q1, *q2;  // column 0 of [N][ldq]
  int ldq;
  const void *wout1, *wout2, *z1, *z2;  // [H] elem, [N][H] elem
  int64_t N;
  int H, act;
  void *dz1, *dz2;  // [N][H] elem
  uint8_t *sel, *sel_out;  // [N]; sel_out may be null
  float* qsel;             // [N]
};
template <class P>
void launch_sac_select(const SacSelect& a, hipStream_t s);

// The chain's tail and the head's backward in one launch.  g[n][j] = sum_k dh[n][k] wa[j][k], k over 2H in index order (fp32 fma;
// the unselected trunk's half is zero): dQ_sel/da.  Then, with the forward's quantities recomputed from the same inputs,
//   dL/du = (1/N) [-g s + alpha 2 a s / (s + 1e-6)],  dL/dmu = dL/du,  dL/dsigma = dL/du zc - alpha / (N sigma),
//   dL/draw = dL/dsigma 0.5 sigma c (1 - tanh(raw)^2)
// into d_out[n][j], d_out[n][AF + j] (elem; the columns from 2 AF to ldd zeroed) and, unrounded, into d_out32[n][.] ([N][2 AF] fp32 or
// null: the heads' bias gradient is its column sum; the sum of bf16-rounded entries costs that gradient 2^-9 / sqrt(N), more than
// rounding every Linear's operands does).  d_a[n][j] = dL/da = (1/N)(-g) or null.
struct SacTail {
  SacHead head;  // cfg, out, noise, AF (its outputs are unused)
  const void* dh;  // [N][2H] elem
  const void* wa;  // [AF][2H] elem
  int H2, rows;    // rows per block: qsm_tail_rows(H2)
  const double* alpha;  // device scalar
  void* d_out;  // [N][ldd] elem
  int ldd;
  float* d_out32;
  float* d_a;
};
template <class P>
void launch_sac_tail(const SacTail& a, hipStream_t s);

// sh[k][0] <- the sum of the 256 threads' v[k], added pairwise in a fixed tree
template <int K>
__device__ __forceinline__ void sac_tree(double (*sh)[256], const double* v) {
  for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    __syncthreads();
  }
}

// stats = {mean(-q_sel + alpha logp), mean q_sel, mean logp, mean sigma}: thread i sums rows i, i + 256, ... in double, the 256
// partials are added pairwise in a fixed tree
struct SacStats {
  const float *qsel, *logp, *sig_row;
  const double* alpha;
  int64_t N;
  int AF;
  double* stats;
};
void launch_sac_stats(const SacStats& a, hipStream_t s);

// loss_critic is idql.h's Q loss with IdqlLoss::next_logp / alpha set:  y = reward + (gamma * (min(tq1, tq2) - alpha next_logp)) *
// (1 - terminated) in fp32;  loss = mean((q1 - y)^2) + mean((q2 - y)^2);  stats = {loss, mean q1, mean y}.

// out = {-alpha (mean logp + target_entropy), the same}: alpha = exp(log_alpha), so d loss / d log_alpha is the loss itself
void launch_sac_alpha_loss(const float* logp, int64_t N, const double* log_alpha, double target_entropy, double* out, hipStream_t s);

}  // namespace dppo
