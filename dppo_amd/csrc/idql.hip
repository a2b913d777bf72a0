// See idql.h.  gfx950 only.  Compiled with -ffp-contract=off: the losses, the bootstrap target and the Polyak average keep the
// reference's op sequence (separate fp32 products and sums, never an fma).
#include "idql.h"

namespace dppo {

int idql_blocks(int64_t N) { return (int)((N + IDQL_RPB - 1) / IDQL_RPB); }

// ---- row builder: one launch writes every operand image of a minibatch ------------------------------------------------------
// (idql_ring_row(), idql.h, maps row n to its position in the ring's storage)
template <class P>
__global__ __launch_bounds__(256) void idql_rows_kernel(const IdqlRows a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;  // elements of one 16-byte store
  const int cQ = a.q1in != nullptr ? a.KpQ / EPC : 0, cV = a.vin != nullptr ? a.KpV / EPC : 0;
  const int cN = a.nvin != nullptr ? a.KpV / EPC : 0, W = cQ + cV + cN;
  const int64_t total = a.N * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / W;
    int c = (int)(i - n * W);
    const int64_t row = idql_ring_row(a, n);
    const int64_t orow = a.obs_mod > 0 ? n % a.obs_mod : row;
    if (c == 0) {
      if (a.r_out != nullptr) a.r_out[n] = a.reward[row];
      if (a.term_out != nullptr) a.term_out[n] = a.terminated[row];
    }
    union {
      E e[EPC];
      u32x4 v;
    } ch;
    if (c < cQ) {  // [obs | action | 0]
#pragma unroll
      for (int k = 0; k < EPC; ++k) {
        const int col = c * EPC + k;
        float x = 0.f;
        if (col < a.OD)
          x = a.obs[orow * a.OD + col];
        else if (col < a.OD + a.AD)
          x = a.actions[row * a.AD + (col - a.OD)];
        ch.e[k] = P::from_f32(x);
      }
      *(u32x4*)((E*)a.q1in + n * a.KpQ + c * EPC) = ch.v;
      if (a.q2in != nullptr) *(u32x4*)((E*)a.q2in + n * a.KpQ + c * EPC) = ch.v;
      continue;
    }
    c -= cQ;
    const bool nxt = c >= cV;
    if (nxt) c -= cV;
    const float* src = (nxt ? a.next_obs : a.obs) + orow * a.OD;
#pragma unroll
    for (int k = 0; k < EPC; ++k) {
      const int col = c * EPC + k;
      ch.e[k] = P::from_f32(col < a.OD ? src[col] : 0.f);
    }
    *(u32x4*)((E*)(nxt ? a.nvin : a.vin) + n * a.KpV + c * EPC) = ch.v;
  }
}
template <class P>
void launch_idql_rows(const IdqlRows& a, hipStream_t s) {
  constexpr int EPC = 16 / P::ESIZE;
  const int W = (a.q1in ? a.KpQ / EPC : 0) + (a.vin ? a.KpV / EPC : 0) + (a.nvin ? a.KpV / EPC : 0);
  int64_t blocks = (a.N * W + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) return;
  hipLaunchKernelGGL((idql_rows_kernel<P>), dim3((unsigned)blocks), dim3(256), 0, s, a);
}
template void launch_idql_rows<F32>(const IdqlRows&, hipStream_t);
template void launch_idql_rows<BF16>(const IdqlRows&, hipStream_t);

// ---- loss epilogues ----------------------------------------------------------------------------------------------------------
// IDQL_RPB rows per block: wave 0 does the per-row arithmetic (one row per lane) and the block's three sums in double, then all
// four waves write the gradient rows (one non-zero column, the GEMM's K padding zeroed) as 16-byte stores.
template <class P>
__device__ __forceinline__ void idql_store_grad(void* dst, int ldd, int64_t row0, int64_t N, const float* g) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const int cpr = ldd / EPC;
  for (int i = threadIdx.x; i < IDQL_RPB * cpr; i += 256) {
    const int r = i / cpr, c = i - r * cpr;
    if (row0 + r >= N) break;
    union {
      E e[EPC];
      u32x4 v;
    } ch;
#pragma unroll
    for (int k = 0; k < EPC; ++k) ch.e[k] = P::from_f32(0.f);
    if (c == 0) ch.e[0] = P::from_f32(g[r]);
    *(u32x4*)((E*)dst + (row0 + r) * ldd + c * EPC) = ch.v;
  }
}
__device__ __forceinline__ void idql_block_sums(double s0, double s1, double s2, double* out) {
  for (int o = 32; o > 0; o >>= 1) s0 += __shfl_down(s0, o), s1 += __shfl_down(s1, o), s2 += __shfl_down(s2, o);
  if (threadIdx.x == 0) out[0] = s0, out[1] = s1, out[2] = s2;
}
// the block partials are added in index order by one lane per statistic: the sums do not depend on how a tree would pair them
__global__ void idql_finalize_kernel(const double* partial, int blocks, int64_t N, double* stats) {
  if (threadIdx.x >= 3) return;
  double s = 0;
  for (int b = 0; b < blocks; ++b) s += partial[4 * b + threadIdx.x];
  stats[threadIdx.x] = s / (double)N;
}

// loss_critic_v (diffusion_idql.py:42-61): adv = min(q1, q2) - v;  loss = mean(where(adv > 0, tau, 1 - tau) * adv^2)
template <class P>
__global__ __launch_bounds__(256) void idql_v_loss_kernel(const IdqlLoss a) {
  __shared__ float g[IDQL_RPB];
  const int64_t row0 = (int64_t)blockIdx.x * IDQL_RPB;
  if (threadIdx.x < IDQL_RPB) {
    const int64_t n = row0 + threadIdx.x;
    const bool live = n < a.N;
    const int64_t nn = live ? n : a.N - 1;
    const float q1 = a.q1[nn * a.ldq];
    const float q = a.q2 != nullptr ? fminf(q1, a.q2[nn * a.ldq]) : q1;
    const float adv = q - a.v[nn * a.ldv];
    const float w = adv > 0.f ? a.tau : 1.f - a.tau;
    const float loss = w * (adv * adv);
    // d mean(w adv^2) / d v = -2 w adv / N
    g[threadIdx.x] = -(2.f * w * adv) / (float)a.N;
    if (live && a.adv_out != nullptr) a.adv_out[n] = adv;
    idql_block_sums(live ? (double)loss : 0.0, live ? (double)adv : 0.0, live && adv > 0.f ? 1.0 : 0.0, a.partial + 4 * blockIdx.x);
  }
  __syncthreads();
  idql_store_grad<P>(a.d_a, a.ldd, row0, a.N, g);
}
template <class P>
void launch_idql_v_loss(const IdqlLoss& a, hipStream_t s) {
  const int blocks = idql_blocks(a.N);
  hipLaunchKernelGGL((idql_v_loss_kernel<P>), dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(idql_finalize_kernel, dim3(1), dim3(64), 0, s, a.partial, blocks, a.N, a.stats);
}
template void launch_idql_v_loss<F32>(const IdqlLoss&, hipStream_t);
template void launch_idql_v_loss<BF16>(const IdqlLoss&, hipStream_t);

// loss_critic_q (diffusion_idql.py:63-87; with v2, diffusion_qsm.py:65-95; with next_logp, gaussian_sac.py:31-59): target = r + gamma * v' * (1 - terminated);  loss = mean((q1 - target)^2) + mean((q2 - target)^2)
template <class P>
__global__ __launch_bounds__(256) void idql_q_loss_kernel(const IdqlLoss a) {
  __shared__ float g1[IDQL_RPB], g2[IDQL_RPB];
  const int64_t row0 = (int64_t)blockIdx.x * IDQL_RPB;
  if (threadIdx.x < IDQL_RPB) {
    const int64_t n = row0 + threadIdx.x;
    const bool live = n < a.N;
    const int64_t nn = live ? n : a.N - 1;
    const float mask = 1.f - a.terminated[nn];
    float nv = a.v[nn * a.ldv];
    if (a.v2 != nullptr) nv = fminf(nv, a.v2[nn * a.ldv]);
    if (a.next_logp != nullptr) {
      const float ent = (float)*a.alpha * a.next_logp[nn];
      nv = nv - ent;
    }
    const float target = a.reward[nn] + (a.gamma * nv) * mask;
    const float q1 = a.q1[nn * a.ldq];
    const float e1 = q1 - target;
    float loss = e1 * e1;
    g1[threadIdx.x] = (2.f * e1) / (float)a.N;
    if (a.q2 != nullptr) {
      const float e2 = a.q2[nn * a.ldq] - target;
      loss += e2 * e2;
      g2[threadIdx.x] = (2.f * e2) / (float)a.N;
    }
    idql_block_sums(live ? (double)loss : 0.0, live ? (double)q1 : 0.0, live ? (double)target : 0.0, a.partial + 4 * blockIdx.x);
  }
  __syncthreads();
  idql_store_grad<P>(a.d_a, a.ldd, row0, a.N, g1);
  if (a.q2 != nullptr) idql_store_grad<P>(a.d_b, a.ldd, row0, a.N, g2);
}
template <class P>
void launch_idql_q_loss(const IdqlLoss& a, hipStream_t s) {
  const int blocks = idql_blocks(a.N);
  hipLaunchKernelGGL((idql_q_loss_kernel<P>), dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(idql_finalize_kernel, dim3(1), dim3(64), 0, s, a.partial, blocks, a.N, a.stats);
}
template void launch_idql_q_loss<F32>(const IdqlLoss&, hipStream_t);
template void launch_idql_q_loss<BF16>(const IdqlLoss&, hipStream_t);

// ---- best-of-N selection (diffusion_idql.py:148-188) --------------------------------------------------------------------------
// 16 lanes per environment: every lane walks the S candidates in index order (the same loads, broadcast), then the 16 lanes copy
// the chosen row.  Mode 0: argmax of min(q1, q2), first index on ties.  Mode 1: s drawn with probability w_s / sum w by
// inverse CDF in index order, w_s = adv_s > 0 ? h : 1 - h.
__global__ __launch_bounds__(256) void idql_select_kernel(const IdqlSelect a) {
  const int sub = threadIdx.x & 15;
  const int64_t b = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (b >= a.B) return;
  int pick = 0;
  if (a.mode == 0) {
    float best = 0.f;
    for (int s = 0; s < a.S; ++s) {
      const int64_t r = (int64_t)s * a.B + b;
      const float q = a.q2 != nullptr ? fminf(a.q1[r], a.q2[r]) : a.q1[r];
      if (s == 0 || q > best) best = q, pick = s;
    }
  } else {
    float total = 0.f;
    for (int s = 0; s < a.S; ++s) {
      const int64_t r = (int64_t)s * a.B + b;
      const float q = a.q2 != nullptr ? fminf(a.q1[r], a.q2[r]) : a.q1[r];
      total += q - a.v[a.v_per_env ? b : r] > 0.f ? a.h : 1.f - a.h;
    }
    float u;
    if (a.u != nullptr) {
      u = a.u[b];
    } else {
      uint32_t c0, c1;
      philox4x32_10((uint64_t)b, a.seed_lo, a.seed_hi, c0, c1);
      u = (float)(c0 >> 8) * 5.9604644775390625e-08f;  // [0, 1) on a 2^-24 grid
    }
    const float thr = u * total;
    float cdf = 0.f;
    pick = a.S - 1;
    for (int s = 0; s < a.S; ++s) {
      const int64_t r = (int64_t)s * a.B + b;
      const float q = a.q2 != nullptr ? fminf(a.q1[r], a.q2[r]) : a.q1[r];
      cdf += q - a.v[a.v_per_env ? b : r] > 0.f ? a.h : 1.f - a.h;
      if (thr < cdf) {
        pick = s;
        break;
      }
    }
  }
  const float* src = a.cand + ((int64_t)pick * a.B + b) * a.AF;
  for (int j = sub; j < a.AF; j += 16) a.actions[b * a.AF + j] = src[j];
  if (sub == 0 && a.idx != nullptr) a.idx[b] = pick;
}
void launch_idql_select(const IdqlSelect& a, hipStream_t s) {
  hipLaunchKernelGGL(idql_select_kernel, dim3((unsigned)((a.B + 15) / 16)), dim3(256), 0, s, a);
}

// ---- Polyak average (diffusion_idql.py:89-95): target <- target * (1 - tau) + source * tau, two fp32 products and one sum -------
__global__ __launch_bounds__(256) void polyak_vec_kernel(f32x4* target, const f32x4* source, float a, float b, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 t = target[i], s = source[i];
    target[i] = t * a + s * b;
  }
}
__global__ __launch_bounds__(256) void polyak_kernel(float* target, const float* source, float a, float b, int64_t i0, int64_t n) {
  for (int64_t i = i0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    target[i] = target[i] * a + source[i] * b;
}
void launch_polyak(float* target, const float* source, float one_minus_tau, float tau, int64_t n, hipStream_t s) {
  const bool vec = ((uintptr_t)target % 16 == 0) && ((uintptr_t)source % 16 == 0);
  const int64_t n4 = vec ? n / 4 : 0;
  if (n4 > 0) {
    const int64_t blocks = (n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048;
    hipLaunchKernelGGL(polyak_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (f32x4*)target, (const f32x4*)source,
                       one_minus_tau, tau, n4);
  }
  const int64_t rest = n - 4 * n4;
  if (rest > 0) {
    const int64_t blocks = (rest + 255) / 256 < 2048 ? (rest + 255) / 256 : 2048;
    hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)blocks), dim3(256), 0, s, target, source, one_minus_tau, tau, 4 * n4, n);
  }
}

}  // namespace dppo
