// LayerNorm in a PLAIN Q trunk: the reference's MLP with use_layernorm (model/common/mlp.py:46-74) puts
// nn.LayerNorm(o_dim) -- eps 1e-5, NOT the residual blocks' 1e-6 (tile_ln.h) -- behind every Linear but the last and in front
// of the activation:  x -> act(LN(W0 x + b0)) -> act(LN(W_b . + b_b)) ... -> Wout . + bout.  This is the critic of every RLPD,
// Cal-QL and IBRL cfg the reference ships (CriticObsAct, use_layernorm: True; double_q: False in RLPD's, True -- a twin, calql.h -- in
// all 16 of Cal-QL's).
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
//
// The actor's loss through the ensemble's mean (reference model/rl/gaussian_rlpd.py:100-112): with a_n, logp_n SAC's reparameterised
// sample at obs_n,  loss = mean_n [-(1/E) sum_e q_e(obs_n, a_n) + alpha logp_n],  g_n = (1/E) sum_e dq_e/da.  The head writes ONE row
// image [obs | a | 0]; every member runs its forward (z, mean, rstd kept) and its own data-gradient chain: the seed Wout (.) act'(z_L),
// then per hidden layer from the top ln_bwd_kernel with no parameter sums and, except at layer 0, the data GEMM with the act' epilogue.
// Member e's dx_0 lands in columns [e H, (e + 1) H) of one [N][E H] image; rlpd_tail_kernel multiplies it with the members' action
// columns of W0, packed as [AF][E H], folds the 1/E in once and runs SAC's head backward with g in place of dQ_sel/da.
//
// Launches of dppo_rlpd_actor_fwd_bwd with L hidden layers per member (read off the code, not traced), side-stream events aside:
//   1 row builder + 1 W0 pack + the actor's forward (3 GEMMs on the shipped two-layer actor) + 1 head epilogue
//   + E x [L x (1 GEMM + 1 row kernel) + 1 GEMM]                  the members' forwards
//   + E x [1 seed + L LayerNorm backwards + (L - 1) data GEMMs]   the members' chains
//   + 1 tail / head backward + 1 statistics (bf16: + 2 for the heads' bias gradient from the unrounded d_out)
//   + the actor's parameter backward.  Nothing of a critic's is written: no weight gradient, column sum or gradient buffer.
//   Shipped halfcheetah (E = 10, L = 2): 4 + 3 + 10 x 5 + 10 x 4 + 2 = 99 before the actor's backward.
// Not built: a member-batched GEMM, weight gradients grouped across members.  (IBRL's model and critic loss: ibrl.h; Cal-QL: calql.h; its actor runs this file's
// chain from a seed of its own: q_chain_from_seed in api.hip.)
//
// Launches of one forward of a trunk: L x (1 GEMM + 1 row kernel) + 1 GEMM.
#pragma once
#include "sac.h"

namespace dppo {

// four consecutive elements of a row as fp32 and back (8 or 16 bytes): the row kernels of this family (ibrl.hip's too)
template <class P>
__device__ __forceinline__ void load4(const typename P::elem_t* p, float (&v)[4]) {
  if constexpr (P::ESIZE == 4) {
    const float4 t = *(const float4*)p;
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    const u32x2 t = *(const u32x2*)p;
    v[0] = bf2f(t.x & 0xffff), v[1] = bf2f(t.x >> 16), v[2] = bf2f(t.y & 0xffff), v[3] = bf2f(t.y >> 16);
  }
}
template <class P>
__device__ __forceinline__ void store4(typename P::elem_t* p, const float (&v)[4]) {
  if constexpr (P::ESIZE == 4) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    u32x2 pk;
    pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    *(u32x2*)p = pk;
  }
}

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
  const float* dz32;  // [M][ld] fp32 or null: the input read from here, unrounded, instead of from dz (ibrl.h); the output still goes to dz
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

// ---- the actor's loss through the ensemble's mean ---------------------------------------------------------------------------------
// (the tail's weight operand [AF][E H] is qsm.h's launch_pack_w0a)
// The chains' tail and the head's backward in one launch.  K = E H is split over RLPD_TAIL_LANES lanes per output (n, j): lane l
// takes the 4-element groups l, l + 16, ... of the row (so the members in index order), one fma per element, and the 16 partials
// are added by a fixed xor butterfly.  Operands come straight from global memory: no LDS tile, so no ceiling on K.  An output
// depends on its own row of dh alone and on nothing of the launch geometry: the same bits in every call, batch size and block.
//   g[n][j] = (sum_k dh[n][k] wa[j][k]) / E,  then sac.h's dL/du, dL/dsigma, dL/draw with g in place of dQ_sel/da.
constexpr int RLPD_TAIL_LANES = 16;
struct RlpdTail {
  SacHead head;    // cfg, out, noise, AF (its outputs are unused)
  const void* dh;  // [N][K] elem, K = E H
  const void* wa;  // [AF][K] elem
  int K, E;
  const double* alpha;  // device scalar
  void* d_out;          // [N][ldd] elem: columns [0, 2 AF) set, the rest zeroed
  int ldd;
  float* d_out32;  // [N][2 AF] fp32 or null: the same before its rounding to elem (SacTail::d_out32)
  float* d_a;      // [N][AF] = -g / N, or null
};
template <class P>
void launch_rlpd_tail(const RlpdTail& a, hipStream_t s);

// stats = {mean(-qm + alpha logp), mean qm, mean logp, mean sigma}, qm[n] = (q_0[n] + q_1[n] + ... in member order) / E in fp32;
// thread i sums rows i, i + 256, ... in double, the 256 partials are added pairwise in a fixed tree (as sac_stats_kernel)
struct RlpdActorStats {
  const float* q;    // member e's Q: column 0 of [N][ldq] at q + e * q_stride
  int64_t q_stride;  // floats
  int ldq, E;
  const float *logp, *sig_row;
  const double* alpha;
  int64_t N;
  int AF;
  double* stats;
};
void launch_rlpd_actor_stats(const RlpdActorStats& a, hipStream_t s);

}  // namespace dppo
