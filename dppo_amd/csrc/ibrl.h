// Imitation-bootstrapped RL (IBRL): the reference's IBRL_Gaussian (model/rl/gaussian_ibrl.py) on the pieces RLPD already has -- the
// flat [E][P] ensemble of LayerNorm Q trunks, their forward and backward, launch_rlpd_loss (rlpd.h) -- plus what is new here.
//
// Dropout in a PLAIN trunk without LayerNorm.  The reference's MLP (model/common/mlp.py:59-60) puts nn.Dropout behind every Linear but
// the last, in front of the activation, and IBRL keeps its three actors in train() while it acts and while it trains: dropout is
// live in the online actor, the frozen bc_policy and target_actor.  The route is the LayerNorm one of mlp_forward: the hidden layer's
// GEMM (launch_gemm_nt, unchanged) leaves its bias-added row unrounded in fp32, drop_rows_kernel then forms
//   z' = keep ? z * (1 / (1 - p)) : 0     in fp32 (torch multiplies by the mask over 1 - p),
// writes act(z') as the next layer's operand and, kept for a backward, z' where the GEMM's epilogue would have put the
// pre-activation.  The mask is applied in front of the activation, never commuted with it (Mish(0) = 0 but Mish(z s) != s Mish(z)).
// The out layer has no dropout.  keep comes from a given mask, uint8 [L][M][H] (L hidden layers, 1 = keep), or from Philox4x32-10
// keyed by (seed_lo, seed_hi) at counter (l M + m) H + h: keep iff u >= p with u = (first word >> 8) 2^-24 in [0, 1).  The mask used
// can be written out ([L][M][H] again), so a drawn call can be repeated from its own mask.
//
// Acting (gaussian_ibrl.py:149-205).  Two proposals per row, the frozen imitation policy's (sigma 1e-4: the reference calls it
// deterministic and still draws) and the online actor's, are scored by the smaller Q of a pair of ONLINE members; the better one, or
// a two-way soft draw, is the action.  min(a, b) is torch.min's: a NaN on either side gives NaN.
//   greedy:  BC iff min q_bc > min q_rl  (strict: a tie or a NaN takes RL, as torch.where does)
//   soft:    w = exp(beta q) for both, p_bc = 1 / (1 + exp(w_rl - w_bc)) in fp32, BC iff u < p_bc; where w_rl - w_bc is NaN (both
//            overflow) the reference's torch.multinomial raises and the greedy rule decides here.
// Launches of dppo_ibrl_act with LA hidden layers in the actor and LQ in a member (read off the code, not traced), dropout on:
//   1 row builder (obs) + 2 actors x [LA x (1 GEMM + 1 dropout row kernel) + 1 GEMM + 1 sample] + 1 row builder (2B rows)
//   + 2 members x [LQ x (1 GEMM + 1 LayerNorm row kernel) + 1 GEMM] + 1 select.
//   Shipped can (LA = LQ = 3): 1 + 2 x 8 + 1 + 2 x 7 + 1 = 33.  Without dropout (halfcheetah) the actors' row kernels fall away: 27.
//   The BC actor and the second member run on a side stream at every B: two fork / join pairs.  Measured at B = 1 on the shipped can
//   shape against the same call on one stream without events: 0.25 against 0.37 ms in fp32; in bf16 0.19 and 0.21 (two runs)
//   against 0.20, which the 5 to 10 % between runs of an unchanged arm does not resolve.
//
// The critics' TD loss (gaussian_ibrl.py:69-113).  The members' rows [obs | a | 0] are written once, the targets' image has 2N rows,
// [s' | a'_bc | 0] then [s' | a'_rl | 0]; each of the two target members of the pair runs ONE forward over the 2N rows.  With
//   mb = min(t1_bc, t2_bc), mr = min(t1_rl, t2_rl):   tq[n] = mb > mr ? mb : mr   (the same strictness)
// RLPD's loss, backwards and out-bias fix run with their launch lists unchanged: launch_rlpd_loss takes t1 = t2 = tq and no entropy
// term.  One difference in bf16: the members' data-gradient GEMMs leave upstream (.) act'(z) in fp32 (MlpBufs::ln_dz32, LnBwd::dz32)
// and LayerNorm's backward reads it from there.  That backward subtracts two projections, so a row rounded to bf16 in front of it
// comes out with more than bf16's error: at N = 1, where nothing averages, a hidden bias gradient was off by 3.2e-3 against 2.0e-3
// without that one rounding (reproduced on the CPU to four digits).  RLPD and Cal-QL leave the buffers null: same bits.
// Launches of dppo_ibrl_q_loss_fwd_bwd with L hidden layers per member (read off the code, not traced), side-stream events aside:
//   1 row builder + 2 target forwards x (2 L + 1) + E forwards x (2 L + 1) + 2 (target, its share) + 3 (loss, statistics, out-layer
//   bias gradients) + E backwards as in rlpd.h.  That is dppo_rlpd_q_loss_fwd_bwd's list plus two.
//
// The actor's loss through the ensemble's MIN (gaussian_ibrl.py:115-128 on GaussianModel.forward, model/common/gaussian.py:85-120).
//   mu = tanh(trunk(obs)) (tanh_mean),  a = mu + sigma clamp(eps, +-c)  (sigma = fixed_std; the reference clamps the sample between
//   bounds that move with mu, so d a / d mu = 1 on every element),  q_e = member_e(obs, a),  m_n = min_e q_e,  loss = -mean_n m_n.
// The min is torch.min's: a NaN Q is the row's min, and A TIE GOES TO THE LOWEST MEMBER INDEX (torch's CPU kernel does the same;
// the reference has no rule of its own).  Only the selected member's dq/da reaches the actor:  d_a = -g / N,  d_u = d_a (1 - mu^2).
// Route (dppo_ibrl_actor_fwd_bwd, the driver beside rlpd_actor_impl):
//   the actor's rows and its forward with the activations kept and dropout live; the mask used goes into the workspace (or the
//   caller's mask_out), so the backward reads the forward's own mask whether it was given or drawn;
//   ibrl_head_kernel: tanh mean, clipped draw, sample, the mean kept, and the ONE critic row image [obs | a | 0];
//   the E members' LayerNorm forwards on the rotating streams; ibrl_min_kernel: per row the argmin, qmin, sel and every member's
//   chain seed Wout (.) act'(z_L), zeroed on the rows it did not win; q_chain_from_seed per member into its columns of [N][E H] (a zero
//   row stays exactly zero through LayerNorm's backward and the data GEMMs, so the tail's sum over K = E H is the selected member's
//   product plus exact zeros); pack_w0a_kernel; ibrl_tail_kernel (rlpd_tail_kernel's 16-lane split of K and xor butterfly, no 1/E)
//   whose epilogue is the head's backward with single-width d_out; ibrl_actor_stats_kernel through sac_tree's fixed order; then the
//   actor's parameter backward, where drop_bwd_kernel turns d/dz' into d/dz = d/dz' keep s in place in front of each hidden
//   layer's weight gradient, column sum and next data GEMM.  The mask is applied explicitly: act'(0) is 0 for ReLU, not for Mish.
//   In bf16 drop_bwd_kernel reads the elem rows the data GEMMs wrote and rounds keep s once more (exact at p = 0.5, where s = 2).
//   Measured at p = 0.25 against the same rows kept in fp32: the worst tensor stays at 1.15 x the bf16-Linear yardstick
//   and 1 - cosine moves from 1.21 x to 1.24 x, against a bound of 2 x, so the fp32 rows the critics' LayerNorm backward needs are
//   not carved here.  The out bias is redone from the unrounded d_out as in sac.h.
// Launches with LA hidden layers in the actor and LQ in a member (read off the code, not traced), side-stream events aside:
//   1 row builder + 1 W0 pack + LA x (1 GEMM + 1 dropout row kernel) + 1 GEMM + 1 head + E x [LQ x (1 GEMM + 1 row kernel) + 1 GEMM]
//   + 1 min/select + E x [LQ LayerNorm backwards + (LQ - 1) data GEMMs] + 1 tail + 1 statistics + the actor's backward with LA
//   dropout backward row kernels (bf16: + 2 for the out bias).  Shipped can (LA = LQ = 3, E = 5): 2 + 7 + 1 + 35 + 1 + 25 + 2 = 73
//   before the actor's backward.  A chain that runs only where a member has rows was not tried.
// Not built: the dropout BC pre-training, a member-batched GEMM, graph capture of the iteration, pixel observations.
#pragma once
#include "rlpd.h"

namespace dppo {

// One wave per row, LN_ROWS_PB rows per block; lane l owns the 4 consecutive features 4 l + 256 k.
struct DropRows {
  const float* x;  // [M][ldx] fp32: the Linear's output, bias added, unrounded
  int ldx;
  int64_t M;
  int H, act;  // H a multiple of 64
  int layer;   // l of the mask's [L][M][H]
  float p, scale;  // scale = 1 / (1 - p)
  uint32_t k0, k1;
  const uint8_t* mask;  // [L][M][H] given, or null: drawn
  uint8_t* mask_out;    // [L][M][H] or null
  void* out_act;        // [M][ldo] elem: act(z')
  void* out_z;          // [M][ldo] elem or null: z'
  int ldo;
};
template <class P>
void launch_drop_rows(const DropRows& a, hipStream_t s);

// Rows of both IBRL entries.  `ring` says where obs / next_obs / actions / reward / terminated come from (idql.h; its outputs are
// unused).  qin (or null) <- [obs | actions | 0], N rows;  tin <- [next_obs | a_bc | 0] at row n and [next_obs | a_rl | 0] at N + n.
struct IbrlRows {
  IdqlRows ring;
  const float *a_bc, *a_rl;  // [N][AD]
  void* qin;                 // [N][Kp] elem or null
  void* tin;                 // [2N][Kp] elem
  int Kp;
  float *r_out, *term_out;  // [N] or null (with qin)
};
template <class P>
void launch_ibrl_rows(const IbrlRows& a, hipStream_t s);

// tq[n] = mb > mr ? mb : mr over column 0 of the two target members' [2N][ldt] outputs; share <- (rows where BC won) / N;
// y_out[n] = reward + (gamma (1 - terminated)) tq, the loss kernel's own arithmetic
struct IbrlTarget {
  const float *t1, *t2;
  int ldt;
  int64_t N;
  float* tq;          // [N]
  const float *reward, *terminated;  // [N] (read with y_out only)
  float gamma;
  float* y_out;       // [N] or null
  uint32_t* partial;  // [ibrl_target_blocks(N)]
  double* share;      // device scalar
};
int ibrl_target_blocks(int64_t N);
void launch_ibrl_target(const IbrlTarget& a, hipStream_t s);

struct IbrlSelect {
  const float *q1, *q2;  // the pair's Q: column 0 of [2N][ldq], rows [0, N) the BC proposal's, [N, 2N) the RL one's
  int ldq;
  int64_t N;
  int AF;
  int soft;
  float beta;
  const float* u;  // [N] or null: Philox keyed by (k0, k1), counter = row
  uint32_t k0, k1;
  const float *a_bc, *a_rl;  // [N][AF]
  float* action;             // [N][AF]
  float *q_bc, *q_rl;        // [N]: the pair's min
  uint8_t* took_bc;          // [N]
};
void launch_ibrl_select(const IbrlSelect& a, hipStream_t s);

// ---- the actor's loss through the ensemble's min ------------------------------------------------------------------------------------
// d/dz' -> d/dz of one hidden layer of a dropout trunk, in place: dz[m][h] = keep ? dz[m][h] * scale : 0 (one wave per row, as DropRows)
struct DropBwd {
  void* dz;           // [M][ld] elem, in and out
  int ld;
  int64_t M;
  int H, layer;
  float scale;
  const uint8_t* mask;  // [L][M][H], 1 = keep
};
template <class P>
void launch_drop_bwd(const DropBwd& a, hipStream_t s);

// One thread per 16-byte chunk of the critic's row image [obs | a | 0]; the thread that owns an action column forms it:
//   mu = tanh_mean ? tanh(out) : out,  a = mu + fixed_std * clamp(z, +-randn_clip),  z given or Philox keyed by the cfg at n AF + j
struct IbrlHead {
  dppo_gaussian_cfg cfg;
  IdqlRows ring;     // where obs comes from; N, OD, AD = AF
  const float* out;  // [N][ldo] the trunk's output
  int ldo;
  const float* noise;   // [N][AF] or null
  float *actions, *mu;  // [N][AF] each
  void* qin;            // [N][Kp] elem
  int Kp;
};
template <class P>
void launch_ibrl_head(const IbrlHead& a, hipStream_t s);

// Per row (one wave): sel = argmin_e q_e (a NaN is the min; a tie goes to the lowest index), qmin, and member e's chain seed
// dz_e[n][h] = elem(wout_e[h] * act'(z_e[n][h])) where e == sel, 0 elsewhere
struct IbrlMin {
  const float* q;    // member e's Q: column 0 of [N][ldq] at q + e * q_stride
  int64_t q_stride;  // floats
  int ldq, E;
  const void* wout[RLPD_MAX_E];  // [H] elem
  const void* z[RLPD_MAX_E];     // [N][H] elem: the last hidden layer's z
  void* dz[RLPD_MAX_E];          // [N][H] elem
  int64_t N;
  int H, act;
  float* qmin;   // [N]
  uint8_t* sel;  // [N]
};
template <class P>
void launch_ibrl_min(const IbrlMin& a, hipStream_t s);

// g[n][j] = sum_k dh[n][k] wa[j][k] (RlpdTail's split of K = E H and butterfly; no 1/E: the seeds carry the choice), then
//   d_a = -g / N,  d_out[n][j] = d_a (1 - mu^2) (tanh_mean) or d_a;  columns [AF, ldd) zeroed
struct IbrlTail {
  const void* dh;  // [N][K] elem
  const void* wa;  // [AF][K] elem
  int K, AF, tanh_mean;
  int64_t N;
  const float* mu;  // [N][AF]
  void* d_out;      // [N][ldd] elem
  int ldd;
  float* d_out32;  // [N][AF] fp32 or null: the same before its rounding to elem
  float* d_a;      // [N][AF] or null
};
template <class P>
void launch_ibrl_tail(const IbrlTail& a, hipStream_t s);

// stats = {-mean qmin, mean qmin, mean over rows and members of q}: rows in double per thread, then sac_tree's fixed order
struct IbrlActorStats {
  const float* qmin;
  const float* q;
  int64_t q_stride;
  int ldq, E;
  int64_t N;
  double* stats;
};
void launch_ibrl_actor_stats(const IbrlActorStats& a, hipStream_t s);

}  // namespace dppo
