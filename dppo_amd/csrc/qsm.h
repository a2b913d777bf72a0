// Q-score matching (QSM): the reference's QSMDiffusion.loss_actor / loss_critic (model/diffusion/diffusion_qsm.py:36-95) around
// the MLP forward every other path uses.  What is new here is the derivative of the twin critic with respect to its ACTION
// input, per row: a row builder (gather, q_sample, both trunks' operand images), the seed of the data-gradient chain
// (d q / d z of the last hidden layer: out_dim is 1, so Wout is broadcast, not multiplied), and the chain's tail, one K = 2H
// product of [dh_0 of Q1 | dh_0 of Q2] with the stacked action columns of the two W0 whose epilogue writes the regression
// target of the actor's denoising MSE.  The critic's TD loss reuses idql.h's Q-loss epilogue with the target twin as bootstrap.
#pragma once
#include "idql.h"

namespace dppo {

// Rows of dppo_qsm_actor_target: `ring` says where obs / actions come from (its outputs are unused).  Per row n:
// x_t = sa[t] * a + sb[t] * noise (two fp32 products, one sum);  pairs[n][0] = x_t;  obs_out[n] = obs;  q1in = q2in = [obs | x_t | 0]
struct QsmRows {
  IdqlRows ring;
  const float* noise;    // [N][AD]
  const int64_t* t;      // [N], clamped into [0, K)
  const float *sa, *sb;  // [K] sqrt(abar), sqrt(1 - abar)
  int K;
  float* pairs;    // [N][2][AD]
  float* obs_out;  // [N][OD]
  void *q1in, *q2in;  // [N][KpQ] elem
  int KpQ;
};
template <class P>
void launch_qsm_rows(const QsmRows& a, hipStream_t s);

// Rows of dppo_qsm_q_loss_fwd_bwd: [obs | action | 0] for the trained twin, [next_obs | next_action | 0] for the target twin
// (next_actions is a plain [N][AD] array: the policy's sample at next_obs), the gathered reward / terminated.
struct QsmTdRows {
  IdqlRows ring;
  const float* next_actions;
  void *q1in, *q2in, *t1in, *t2in;  // [N][KpQ] elem
  int KpQ;
  float *r_out, *term_out;
};
template <class P>
void launch_qsm_td_rows(const QsmTdRows& a, hipStream_t s);

// dz[n][h] = elem(wout[h] * act'(z[n][h])): d q / d (pre-activation of the last hidden layer) of a trunk with one output
template <class P>
void launch_qsm_seed(const void* wout, const void* z, int64_t N, int H, int act, void* dz, hipStream_t s);

// wa[a][e * H + h] = elem(W0 of trunk e [h][OD + a]), e < E (trunk e's flat image starts at params + e * stride): [AF][E H], the
// weight operand of every tail (the twins' at E = 2, RLPD's members')
template <class P>
void launch_pack_w0a(const float* params, int64_t stride, int64_t w0_off, int in_dim, int OD, int AF, int H, int E, void* wa,
                     hipStream_t s);

// g[n][a] = 0.5 * sum_k dh[n][k] wa[a][k], k over 2H in index order (fp32 fma);  pairs[n][1][a] = -coeff * g;  g_out[n][a] = g
struct QsmTail {
  const void* dh;  // [N][2H] elem
  const void* wa;  // [AD][2H] elem
  int64_t N;
  int H2, AD, rows;  // rows per block: qsm_tail_rows(H2)
  float coeff;
  float* pairs;  // [N][2][AD]
  float* g_out;  // [N][AD] or null
};
int qsm_tail_rows(int H2);  // 0: 2H too wide for the LDS tile
template <class P>
void launch_qsm_tail(const QsmTail& a, hipStream_t s);

}  // namespace dppo
