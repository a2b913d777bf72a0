// Cal-QL's conservative critic loss (reference model/rl/gaussian_calql.py:56-171) on a TWIN of the LayerNorm Q trunks of rlpd.h: the
// critic of all 16 calql_mlp_*.yaml the reference ships (CriticObsAct, use_layernorm: True, double_q: True).
//
// Notation: N batch, R random actions per row, S policy samples per next observation, AF = Ta Da, c = 0.5^AF (the literal value the
// reference subtracts as "log_rand_pi"; not a logarithm, imitated), w = cql_min_q_weight.
//   target (no gradient)  next_q[n] = max_s min(tq1, tq2)(next_obs_n, a'_{n,s}),  y = r + (gamma (1 - terminated)) next_q
//   per trunk i           qd = q_i(obs, actions),  td_i = mean((qd - y)^2)
//                         q_rand[n][r] = q_i(obs_n, random_actions[n][r]) - c
//                         A[n] = max(q_i(obs_n, pi_a_n), returns_n),  A'[n] = max(q_i(next_obs_n, pi_next_a_n), returns_n)
//                         ood[n] = logsumexp([q_rand[n][:], A[n] + o_n, A'[n] + o'_n]),  diff_i = clamp(ood - qd, lo, hi)
//   loss = td_1 + td_2 + w mean(diff_1) + w mean(diff_2)
// The reference's broadcast.  It subtracts log_pi (N,) from A[:, None] (N, 1): the result is (N, N), and row n of its (N, R + 2 N)
// matrix holds A[n] - log_pi[m] for EVERY m of the batch.  logsumexp_m(A_n - lp_m) = A_n + logsumexp_m(-lp_m), so its loss is the
// line above with o_n = L = logsumexp_m(-log_pi[m]) and o'_n = L' = logsumexp_m(-log_pi_next[m]): two scalars per batch
// (per_row_logpi = 0, the default; calql_lse_kernel).  per_row_logpi = 1 takes o_n = -log_pi[n], o'_n = -log_pi_next[n], the Cal-QL
// paper's importance weights; the same loss kernel with a per-row offset.
// Gradient rows, g = w / N where lo <= ood - qd <= hi (torch.clamp's inclusive rule) and 0 elsewhere, p the softmax of the R + 2
// entries: data 2 (qd - y) / N - g; random r: g p_r; pi: g p_R where q > returns, half at equality (torch.max's rule), 0 below;
// pi_next likewise with p_{R+1}.  log_pi is data: nothing reaches the actor.
//
// The row builder writes ONE image of M = N (R + 3) critic rows [obs | a | 0] that both trunks read, in four segments -- data [0, N),
// random [N, N + N R) (row N + n R + r), pi [N + N R, +N) and pi_next (on next_obs) [N + N R + N, +N) -- and the target twin's N S rows
// [next_obs_n | a'_{n,s}] (row n S + s).  Each trunk runs its forward ONCE over the M rows and its LayerNorm backward once over M rows
// (mlp_forward / mlp_backward, as a member of rlpd.h's ensemble); Q2 and the two target trunks run on the library's side streams.
//
// Launches of dppo_calql_q_loss_fwd_bwd with L = n_blocks + 1 hidden layers (read off the code, not traced), side-stream events
// aside: 1 row builder + [1 reduction for L, L' unless per_row_logpi] + 2 target forwards x (2 L + 1) + 2 forwards x (2 L + 1)
//        + 1 target + 2 (loss, statistics) + 2 backwards x [1 data GEMM + L x (2 LayerNorm backward + weight gradient + its slab
//          reduce + 2 column sum) + (L - 1) data GEMMs + out layer's weight gradient, slab reduce and 2 column sum] + 1 out-layer bias.
//   Shipped kitchen (L = 3): 1 + 1 + 14 + 14 + 3 + 2 x 25 + 1 = 84.
//
// The actor's loss through the twin's minimum (reference model/rl/gaussian_calql.py:173-182): with a_n, logp_n SAC's reparameterised
// sample at obs_n,  loss = mean_n [-min(q1, q2)(obs_n, a_n) + alpha logp_n].  The head writes ONE row image [obs | a | 0] that both
// trunks read; each runs its forward (z, mean, rstd kept).  calql_select_kernel picks per row (q2 < q1: Q2; q1 == q2: both at one
// half, torch.minimum's backward; everything else, a NaN included: Q1) and writes both chains' seeds w_i Wout_i (.) act'(z_L), zero
// for the trunk a row did not select.  From there each trunk runs rlpd.h's data-gradient chain (q_chain_from_seed, shared with
// dppo_rlpd_actor_fwd_bwd): per hidden layer from the top ln_bwd_kernel with no parameter sums and, except at layer 0, the data GEMM
// with the act' epilogue.  Trunk i's dx_0 lands in columns [i H, (i + 1) H) of one [N][2H] image; launch_pack_w0a (E = 2) packs
// the action columns of both W0 as [AF][2H]; launch_rlpd_tail with K = 2H, E = 1 forms g = dQ_sel/da (the unselected half is zero,
// a tie's halves add) and runs SAC's head backward; launch_sac_stats on qsel gives {loss, mean qsel, mean logp, mean sigma}.
//
// Launches of dppo_calql_actor_fwd_bwd with L hidden layers per trunk (read off the code, not traced), side-stream events aside:
//   1 row builder + 1 W0 pack + the actor's forward (3 GEMMs on the shipped two-layer actor) + 1 head epilogue
//   + 2 x [L x (1 GEMM + 1 row kernel) + 1 GEMM]          the trunks' forwards (Q2 on a side stream)
//   + 1 select/seed
//   + 2 x [L LayerNorm backwards + (L - 1) data GEMMs]    the trunks' chains (Q2 on a side stream)
//   + 1 tail / head backward + 1 statistics (bf16: + 2 for the heads' bias gradient from the unrounded d_out)
//   + the actor's parameter backward.  Nothing of the critic's is written: no weight gradient, column sum or gradient buffer.
//   Shipped kitchen (L = 3): 2 + 3 + 1 + 2 x 7 + 1 + 2 x 5 + 2 = 33 before the actor's backward.
// Not built: a member-batched or fused twin chain.  (IBRL's model and critic loss: ibrl.h.)
#pragma once
#include "rlpd.h"

namespace dppo {

constexpr int CALQL_MAX_SAMPLES = 64;  // R and S: the loss kernel keeps a row's R + 3 gradient values per lane in LDS

struct CalqlRows {
  IdqlRows ring;                // obs, next_obs, actions, reward, terminated of the N transitions
  const float* random_actions;  // [N R][AF], or null: drawn here
  const float *pi_actions, *pi_next_actions;  // [N][AF]
  const float* next_actions;                  // [N S][AF]
  int R, S;
  uint32_t seed_lo, seed_hi;
  void* qin;  // [N (R + 3)][KpQ] elem
  void* tin;  // [N S][KpQ] elem
  int KpQ;
  float *r_out, *term_out;  // [N]
  float* random_out;        // [N R][AF] or null
};
template <class P>
void launch_calql_rows(const CalqlRows& a, hipStream_t s);

// out[0] = logsumexp_m(-log_pi[m]), out[1] = logsumexp_m(-log_pi_next[m]): one block each, thread i takes rows i, i + 256, ..., the
// 256 partials are combined pairwise in a fixed tree (the maximum, then the sum of exp in double)
void launch_calql_lse(const float* log_pi, const float* log_pi_next, int64_t N, float* out, hipStream_t s);

// y[n] = reward + (gamma (1 - terminated)) max_s min(t1, t2)[n S + s]; one thread per row
void launch_calql_target(const float* t1, const float* t2, int ldt, const float* reward, const float* terminated, float gamma,
                         int64_t N, int S, float* y, float* y_out, hipStream_t s);

struct CalqlLoss {
  const float* q;    // trunk i's Q over the M rows: column 0 of [M][ldq] at q + i * q_stride
  int64_t q_stride;  // floats
  int ldq;
  const float *y, *returns;          // [N]
  const float *log_pi, *log_pi_next; // [N]
  const float* lse;                  // {L, L'} (per_row_logpi = 0)
  int per_row;
  float w, clip_min, clip_max, c;
  int64_t N;
  int R;
  void* d_out;       // trunk i's gradient rows [M][ldd] elem at (char*)d_out + i * d_stride: column 0 set, the rest zeroed
  int64_t d_stride;  // bytes
  int ldd;
  double* partial;   // [2][blocks][4]: sums of (qd - y)^2, qd, y and of ALL the block's gradient rows (launch_rlpd_out_bias reads it)
  double* partial_d; // [2][blocks]: sums of the clamped differences
  double* stats;     // [6] {loss, td_1 + td_2, mean diff_1, mean diff_2, mean q1 (data rows), mean y}
};
template <class P>
void launch_calql_loss(const CalqlLoss& a, hipStream_t s);

// ---- the actor's loss through the twin's minimum -----------------------------------------------------------------------------------
// sel[n] = 1 where q2 < q1 (weights 0, 1), 2 where q1 == q2 (weights 1/2, 1/2: torch.minimum's backward), 0 otherwise (weights 1, 0;
// a NaN on either side lands here);  qsel[n] = q2 where sel = 1, q1 elsewhere (no fminf: a NaN in q1 reaches the statistics);
// dz_i[n][h] = elem(w_i * (wout_i[h] * act'(z_i[n][h]))), exactly zero for w_i = 0.  The whole [N][H] image of both trunks is written
// on every call.  One wave per row, CALQL_SEL_ROWS rows per 256-thread block, 16-byte accesses along H (a multiple of 64).
constexpr int CALQL_SEL_ROWS = 4;
struct CalqlSelect {
  const float *q1, *q2;  // column 0 of [N][ldq]
  int ldq;
  const void *wout1, *wout2, *z1, *z2;  // [H] elem, [N][H] elem: the top hidden layer's LayerNorm output z
  int64_t N;
  int H, act;
  void *dz1, *dz2;  // [N][H] elem
  uint8_t* sel;     // [N]
  float* qsel;      // [N]
};
template <class P>
void launch_calql_select(const CalqlSelect& a, hipStream_t s);

}  // namespace dppo
