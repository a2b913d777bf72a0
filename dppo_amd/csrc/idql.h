// Implicit diffusion Q-learning (IDQL): the reference's IDQLDiffusion.loss_critic_v / loss_critic_q / update_target_critic /
// forward (model/diffusion/diffusion_idql.py:42-95, 125-188) as a row builder over a device-resident replay ring, two loss
// epilogues, a best-of-N selection kernel and the Polyak average, around the MLP forward / backward every other path uses.
#pragma once
#include "common.h"
#include "dppo_hip.h"

namespace dppo {

constexpr int IDQL_RPB = 64;  // rows per 256-thread block of the loss epilogues

// Where the rows of a minibatch come from: the replay ring (batch != null; row n is logical index inds[n], or n) or, for
// dppo_idql_q_forward, plain arrays with the observation of row n taken from row n % obs_mod.
struct IdqlRows {
  const float *obs, *next_obs, *actions, *reward, *terminated;
  const int64_t* inds;
  int64_t cap, E, head, count;  // count: stored steps (logical indices live in [0, count * E))
  int64_t obs_mod;              // > 0: no ring; obs row n % obs_mod, action row n
  int64_t N;
  int OD, AD;
  // outputs (any may be null): [obs | action] rows for Q1 and Q2, obs rows, next_obs rows (elem, padded with zeros), and the
  // gathered per-row reward / terminated
  void *q1in, *q2in, *vin, *nvin;
  int KpQ, KpV;
  float *r_out, *term_out;
};
template <class P>
void launch_idql_rows(const IdqlRows& a, hipStream_t s);
// Position in the ring's storage of the transition behind row n: logical index l = inds[n] (or n) counts "s e -> (s e)" over
// the stored steps, oldest first; step s lives in slot (head + s) % cap.  An index outside the stored range is clamped into
// it (the indices come from the host's generator; a stale one must not read outside the ring).
__device__ __forceinline__ int64_t idql_ring_row(const IdqlRows& a, int64_t n) {
  if (a.obs_mod > 0) return n;
  int64_t l = a.inds != nullptr ? a.inds[n] : n;
  const int64_t top = a.count * a.E - 1;
  l = l < 0 ? 0 : (l > top ? top : l);
  const int64_t st = l / a.E, e = l - st * a.E;
  return ((a.head + st) % a.cap) * a.E + e;
}

struct IdqlLoss {
  const float *q1, *q2, *v;  // trunk outputs, column 0 of [N][ld]
  const float* v2;           // Q loss, or null: the bootstrap value is min(v, v2) (a target twin on the next rows: qsm.h)
  const float* next_logp;    // Q loss, or null: [N]; the bootstrap value less alpha * next_logp[n] (the entropy term: sac.h)
  const double* alpha;       // device scalar, read only with next_logp
  int ldq, ldv;
  const float *reward, *terminated;  // [N] (Q loss)
  int64_t N;
  float tau, gamma;
  void *d_a, *d_b;  // V loss: d_a = d loss / d v.  Q loss: d_a, d_b = d loss / d q1, q2.  [N][ldd] elem, pad columns zeroed
  int ldd;
  float* adv_out;   // [N] or null (V loss)
  double* partial;  // [blocks][4]
  double* stats;    // [3]
};
int idql_blocks(int64_t N);
template <class P>
void launch_idql_v_loss(const IdqlLoss& a, hipStream_t s);
template <class P>
void launch_idql_q_loss(const IdqlLoss& a, hipStream_t s);

struct IdqlSelect {
  const float *q1, *q2, *v;  // [S*B] sample-major; q2 may be null; v [S*B], or [B] with v_per_env
  const float* cand;         // [S*B][AF]
  const float* u;            // [B] or null
  int64_t B;
  int S, AF, mode, v_per_env;
  float h;
  uint32_t seed_lo, seed_hi;
  float* actions;  // [B][AF]
  int32_t* idx;    // [B]
};
void launch_idql_select(const IdqlSelect& a, hipStream_t s);
void launch_polyak(float* target, const float* source, float one_minus_tau, float tau, int64_t n, hipStream_t s);

}  // namespace dppo
