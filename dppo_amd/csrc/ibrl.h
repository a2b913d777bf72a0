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
// Not built: loss_actor (the min over E members, the backward through dropout, a fixed-std tanh-mean head backward), a member-batched
// GEMM.
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

}  // namespace dppo
