// LayerNorm in a PLAIN Q trunk: the reference's MLP with use_layernorm (model/common/mlp.py:46-74) puts
// nn.LayerNorm(o_dim) -- eps 1e-5, NOT the residual blocks' 1e-6 (tile_ln.h) -- behind every Linear but the last and in front
// of the activation:  x -> act(LN(W0 x + b0)) -> act(LN(W_b . + b_b)) ... -> Wout . + bout.  This is the critic of every RLPD,
// Cal-QL and IBRL cfg the reference ships (CriticObsAct, use_layernorm: True, double_q: False).
//
// Forward.  The hidden layer's GEMM (launch_gemm_nt, unchanged) writes its bias-added row in fp32 with no activation;
// ln_rows_kernel then normalises the unrounded row and applies the activation.  It keeps what the backward needs: z = xhat * gamma
// + beta as elem (the source of the existing dsrc / dact epilogue) and mean / rstd per row; the pre-LayerNorm row stays in fp32.
// Backward.  The existing data-gradient GEMM yields dz = upstream (.) act'(z); ln_bwd_kernel turns it, in place, into
//   dx = rstd (gamma dz - mean_j(gamma dz) - xhat mean_j(gamma dz xhat))
// which feeds weight_grad, launch_colsum and the next data GEMM unchanged, and sums dgamma = sum_m dz xhat, dbeta = sum_m dz in two
// fixed-order stages (per wave in registers, the block's four waves through LDS in wave order, then the blocks in index order by
// ln_bwd_finalize_kernel): the same inputs give the same bits.
//
// The ensemble's TD loss (reference model/rl/gaussian_rlpd.py:64-103).  E members share one descriptor and sit in one flat fp32
// buffer [E][P] with one kernel image each; the target ensemble has the same layout.  Only the two target members of the pair run:
//   y = r + (gamma (1 - term)) min(tq_i, tq_j)  [+ ((gamma (1 - term)) alpha) (-next_logp)],   loss = mean over E N of (q_e - y)^2,
// member e's gradient row is 2 (q_e - y) / (E N), and all E parameter backwards write into one [E][P] gradient.
//
// Launches of dppo_rlpd_q_loss_fwd_bwd with L = n_blocks + 1 hidden layers (read off the code, not traced), side-stream events
// aside: 1 row builder + 2 target forwards x (2 L + 1) + E forwards x (2 L + 1) + 3 (loss, statistics, out-layer bias gradients)
//        + E backwards x [1 data GEMM + L x (2 LayerNorm backward + weight gradient + its slab reduce + 2 column sum) + (L - 1)
//          data GEMMs + out layer's weight gradient, slab reduce and 2 column sum].
// The members' GEMMs go through launch_gemm_nt / weight_grad once per member, spread over the side streams.
// Not built: the actor's call through the ensemble's mean, a member-batched GEMM, weight gradients grouped across members.
//
// Launches of one forward of a trunk: L x (1 GEMM + 1 row kernel) + 1 GEMM.
#pragma once
#include "common.h"

namespace dppo {

constexpr float PLAIN_LN_EPS = 1e-5f;  // nn.LayerNorm's default
constexpr int LN_ROWS_PB = 4;          // rows per 256-thread block: one wave per row

struct LnRows {
  const float* x;  // [M][ldx] fp32: the Linear's output, bias added, unrounded
  int ldx;
  const float *gamma, *beta;  // [H] each, in the fp32 parameter image (any 4-byte alignment)
  int64_t M;
  int H, act;     // H a multiple of 64
  void* out_act;  // [M][ldo] elem: act(z), the next layer's operand
  void* out_z;    // [M][ldo] elem or null: z, kept for the backward
  int ldo;
  float* stats;  // [M][2] {mean, rstd} or null
};
template <class P>
void launch_ln_rows(const LnRows& a, hipStream_t s);

constexpr int LN_BWD_ROWS = 32;  // rows per 256-thread block: 8 per wave, one after the other
constexpr int LN_MAX_H = 1024;   // a lane keeps its columns' parameter sums in registers: 4 x 4 columns
struct LnBwd {
  void* dz;  // [M][ld] elem.  In: upstream (.) act'(z).  Out (in place; a lane reads an element before it writes it): d loss / d x
  int ld;
  const float* x;  // [M][ldx] fp32: the pre-LayerNorm rows the forward's GEMM left
  int ldx;
  const float* stats;  // [M][2] {mean, rstd}
  const float* gamma;  // [H]
  int64_t M;
  int H;
  float* partial;          // [ln_bwd_blocks(M)][2][H], or null: no parameter sums (a data-gradient chain)
  float *dgamma, *dbeta;   // [H] each
};
int ln_bwd_blocks(int64_t M);
template <class P>
void launch_ln_bwd(const LnBwd& a, hipStream_t s);

constexpr int RLPD_RPB = 64;  // rows per block of the loss epilogue (wave 0: one row per lane)
constexpr int RLPD_MAX_E = 16;
struct RlpdLoss {
  const float* q;    // member e's Q: column 0 of [N][ldq] at q + e * q_stride
  int64_t q_stride;  // floats
  int ldq;
  const float *t1, *t2;  // the pair's target Q: column 0 of [N][ldt]
  int ldt;
  const float *reward, *terminated;  // [N]
  const float* next_logp;            // [N], or null: no entropy backup
  const double* alpha;               // device scalar (read with next_logp only)
  float gamma;
  int64_t N;
  int E;
  void* d_out;       // member e's gradient rows [N][ldd] elem at (char*)d_out + e * d_stride: column 0 set, the rest zeroed
  int64_t d_stride;  // bytes
  int ldd;
  double* partial;  // [E][blocks][4]: sums of (q - y)^2, q, y and of the gradient rows
  double* stats;    // {loss, mean q, mean y}
};
int rlpd_blocks(int64_t N);
template <class P>
void launch_rlpd_loss(const RlpdLoss& a, hipStream_t s);
// grad[e * stride + bout] <- member e's out-layer bias gradient from the loss kernel's fourth partial: the sum of the UNROUNDED
// gradient rows.  The column sum of the elem rows costs that gradient 2^-9 per row in bf16 (at N = 1 all of it), more than
// rounding every Linear's operands does; run behind the members' backwards, whose column sum it overwrites.
void launch_rlpd_out_bias(const double* partial, int64_t N, int E, float* grad, int64_t stride, int64_t bout, hipStream_t s);

}  // namespace dppo
