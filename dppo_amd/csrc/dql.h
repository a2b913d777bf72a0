// Diffusion Q-learning (DQL): the reference's DQLDiffusion.loss_actor (model/diffusion/diffusion_dql.py:74-88, forward_train
// :141-179) -- the one loss whose gradient flows THROUGH the sampler.  The call consumes a stored chain x_K .. x_0, so every
// network input of every step is known: one batched forward over (K + 1) N rows (K chain slabs, step-major, plus the slab of the
// behaviour-cloning term's x_noisy) keeps the activations, and only the gradient with respect to x walks the chain step by step.
// What is new here: the row builder, the posterior epilogue (x0_raw, the clamp mask), the BC loss on the last slab, the fixed-order
// statistics that also leave the critic seed's scale on the device, and the chain's link -- a K = H product of a slab's dh_0 with
// the x columns of W0 whose epilogue applies the posterior's two terms and writes d eps of the next slab.
#pragma once
#include "idql.h"

namespace dppo {

// Rows.  Actor row s * N + n, s < K: [x_s | temb(K - 1 - s) | obs | 0] with x_s = chains[n][s];  s = K: x = sa[t] a + sb[t] noise
// (two fp32 products, one sum; a = chains[n][K], t = t_bc[n] clamped into [0, K)).  krow = the row's diffusion time.  With an
// observation encoder the state columns stay zero (cond_encode fills them) and inC gets [obs | 0].  Critic rows: [obs | a | 0].
struct DqlRows {
  IdqlRows ring;  // where the observations come from (its outputs are unused)
  const float* chains;    // [N][K + 1][AF]
  const float* noise_bc;  // [N][AF]
  const int64_t* t_bc;    // [N]
  const float *sa, *sb;   // [K]
  const float* temb;      // [K][td]
  int K, AF, td, obs_in_a;
  void* inA;  // [(K + 1) N][KpA] elem
  int KpA;
  void* inC;  // [(K + 1) N][KpC] elem, or null
  int KpC;
  int32_t* krow;      // [(K + 1) N]
  void *q1in, *q2in;  // [N][KpQ] elem
  int KpQ;
};
template <class P>
void launch_dql_rows(const DqlRows& a, hipStream_t s);

// mask[n][s][j] = 1 where |c0 x - c1 eps| <= clip (or no clip is configured): the elements the x0 clamp of step s passes
struct DqlPost {
  const float* chains;
  const float* eps;  // the forward's output, [(K + 1) N][lde]
  int lde;
  const dppo_step* tsteps;  // [K], entry t = the coefficients of diffusion time t
  int64_t N;
  int K, AF, has_clip;
  float clip;
  uint8_t* mask;  // [N][K][AF]
};
void launch_dql_post(const DqlPost& a, hipStream_t s);

// The BC term on slab K: rowsum[n] = sum_j (eps - noise)^2 in double, d_out = elem(2 (eps - noise) / (N AF))
struct DqlBc {
  const float* eps;  // slab K of the forward's output
  int lde;
  const float* noise;  // [N][AF]
  int64_t N;
  int AF;
  void* d_out;  // slab K, [N][ldd] elem
  int ldd;
  double* rowsum;  // [N]
};
template <class P>
void launch_dql_bc(const DqlBc& a, hipStream_t s);

// One block, fixed order, doubles: stats = {loss, bc, q_loss, mean q1, mean q2} with q_loss = -mean(q_i) / mean|q_j|, i = which,
// j = 1 - which, loss = bc + eta q_loss;  *scale = (float)(-eta / (N mean|q_j|)), the factor of dQ_i/da in the seed
struct DqlStats {
  const float *q1, *q2;  // column 0 of [N][ldq]
  int ldq;
  const double* rowsum;
  int64_t N;
  int AF, which;
  double eta;
  double* stats;
  float* scale;
};
void launch_dql_stats(const DqlStats& a, hipStream_t s);

// wa[j][h] = elem(W0[h][col0 + j]), j < ncols: the columns of a first layer that multiply x (actor) or the action (critic)
template <class P>
void launch_dql_pack_cols(const float* w0, int in_dim, int col0, int ncols, int H, void* wa, hipStream_t s);

// The chain's link.  acc[n][j] = sum_k dh[n][k] wa[j][k], k in index order (fp32 fma), one output per thread; then
//   mode 0 (critic seed):  v = *scale * acc
//   mode 1 (BC seed):      v = dx + sa[t_bc[n]] * acc;  d_a = v;  with final_clip, v = 0 where |a| >= 1
//   mode 2 (step at chain position p, time t):  v = (c3 + c2 c0 m[n][p][j]) dx + acc
// dx <- v, and (d_out_prev != null) d eps of the step before, d_out_prev[n][j] = elem(-(c1' c2') m[n][p - 1][j] v).
struct DqlLink {
  const void* dh;  // [N][ldh] elem
  int ldh;
  const void* wa;  // [AF][H] elem
  int64_t N;
  int H, AF, rows, mode;
  float* dx;  // [N][AF]
  const float* scale;
  const int64_t* t_bc;
  const float* sa;
  const float* a;  // chains + K * AF (row stride (K + 1) AF)
  int K, final_clip, p;
  float* d_a;  // [N][AF] or null
  const dppo_step* tsteps;  // [K] by diffusion time: the step at position p has t = K - 1 - p, the one before it t' = K - p
  const uint8_t* mask;
  void* d_out_prev;  // [N][ldd] elem
  int ldd;
};
template <class P>
void launch_dql_link(const DqlLink& a, hipStream_t s);

}  // namespace dppo
