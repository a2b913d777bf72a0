// See calql.h.  gfx950 only.  Compiled with -ffp-contract=off: the loss keeps torch's op sequence (separate products and sums).
#include "calql.h"

namespace dppo {

template <class P>
union CalqlChunk {
  typename P::elem_t e[16 / P::ESIZE];
  u32x4 v;
};

// ---- row builder --------------------------------------------------------------------------------------------------------------
// One thread per 16-byte chunk of a row's operand image, the critic's M rows first, then the target's N S.  The thread that owns an
// action column of a random row also writes its fp32 copy (random_out): every column of [obs | a] is below in_dim <= KpQ, so each
// is written exactly once.  A draw is the top 24 bits of Philox's first word, counter = the element's index in (N R, AF): u in
// [0, 1) exactly, 2 u - 1 in [-1, 1).
template <class P>
__global__ __launch_bounds__(256) void calql_rows_kernel(const CalqlRows a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const IdqlRows& g = a.ring;
  const int W = a.KpQ / EPC, OD = g.OD, AD = g.AD, R = a.R, S = a.S;
  const int64_t N = g.N, NR = N * R, M = N * (R + 3);
  const int64_t total = (M + N * S) * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / W;
    const int c = (int)(i - m * W);
    int64_t n, k = 0;  // the transition, and the row of the action's source
    int seg;           // 0 data, 1 random, 2 pi, 3 pi_next, 4 target
    if (m < N)
      seg = 0, n = m;
    else if (m < N + NR)
      seg = 1, k = m - N, n = k / R;
    else if (m < N + NR + N)
      seg = 2, n = m - N - NR, k = n;
    else if (m < M)
      seg = 3, n = m - N - NR - N, k = n;
    else
      seg = 4, k = m - M, n = k / S;
    const int64_t row = idql_ring_row(g, n);
    if (seg == 0 && c == 0) {
      a.r_out[n] = g.reward[row];
      a.term_out[n] = g.terminated[row];
    }
    const float* ob = (seg >= 3 ? g.next_obs : g.obs) + row * OD;
    const float* ac = seg == 0   ? g.actions + row * AD
                      : seg == 1 ? (a.random_actions != nullptr ? a.random_actions + k * AD : nullptr)
                      : seg == 2 ? a.pi_actions + k * AD
                      : seg == 3 ? a.pi_next_actions + k * AD
                                 : a.next_actions + k * AD;
    CalqlChunk<P> ch;
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int col = c * EPC + e;
      float x = 0.f;
      if (col < OD) {
        x = ob[col];
      } else if (col < OD + AD) {
        const int j = col - OD;
        if (ac != nullptr) {
          x = ac[j];
        } else {
          uint32_t c0, c1;
          philox4x32_10((uint64_t)(k * AD + j), a.seed_lo, a.seed_hi, c0, c1);
          x = (float)(c0 >> 8) * 1.1920928955078125e-07f;  // 2^-23: 2 u with u = (c0 >> 8) 2^-24
          x = x - 1.f;
        }
        if (seg == 1 && a.random_out != nullptr) a.random_out[k * AD + j] = x;
      }
      ch.e[e] = P::from_f32(x);
    }
    E* dst = seg == 4 ? (E*)a.tin + (m - M) * a.KpQ : (E*)a.qin + m * a.KpQ;
    *(u32x4*)(dst + c * EPC) = ch.v;
  }
}
template <class P>
void launch_calql_rows(const CalqlRows& a, hipStream_t s) {
  const int64_t items = a.ring.N * (a.R + 3 + a.S) * (a.KpQ / (16 / P::ESIZE));
  if (items < 1) return;
  const int64_t blocks = (items + 255) / 256;
  hipLaunchKernelGGL((calql_rows_kernel<P>), dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, s, a);
}
template void launch_calql_rows<F32>(const CalqlRows&, hipStream_t);
template void launch_calql_rows<BF16>(const CalqlRows&, hipStream_t);

// ---- L = logsumexp_m(-log_pi[m]) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void calql_lse_kernel(const float* log_pi, const float* log_pi_next, int64_t N, float* out) {
  __shared__ float smax[256];
  __shared__ double ssum[256];
  const float* x = blockIdx.x ? log_pi_next : log_pi;
  float mx = -INFINITY;
  for (int64_t n = threadIdx.x; n < N; n += 256) mx = fmaxf(mx, -x[n]);
  smax[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + w]);
    __syncthreads();
  }
  mx = smax[0];
  double sum = 0.0;
  for (int64_t n = threadIdx.x; n < N; n += 256) sum += (double)expf(-x[n] - mx);
  ssum[threadIdx.x] = sum;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) ssum[threadIdx.x] += ssum[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = logf((float)ssum[0]) + mx;
}
void launch_calql_lse(const float* log_pi, const float* log_pi_next, int64_t N, float* out, hipStream_t s) {
  hipLaunchKernelGGL(calql_lse_kernel, dim3(2), dim3(256), 0, s, log_pi, log_pi_next, N, out);
}

// ---- target -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void calql_target_kernel(const float* t1, const float* t2, int ldt, const float* reward,
                                                            const float* terminated, float gamma, int64_t N, int S, float* y,
                                                            float* y_out) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float nq = -INFINITY;
  for (int s = 0; s < S; ++s) {
    const int64_t k = (n * S + s) * ldt;
    nq = fmaxf(nq, fminf(t1[k], t2[k]));
  }
  const float m = gamma * (1.f - terminated[n]);
  const float v = reward[n] + m * nq;
  y[n] = v;
  if (y_out != nullptr) y_out[n] = v;
}
void launch_calql_target(const float* t1, const float* t2, int ldt, const float* reward, const float* terminated, float gamma,
                         int64_t N, int S, float* y, float* y_out, hipStream_t s) {
  hipLaunchKernelGGL(calql_target_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, t1, t2, ldt, reward, terminated, gamma,
                     N, S, y, y_out);
}

// ---- the loss ---------------------------------------------------------------------------------------------------------------------
// blockIdx.y is the trunk, a block takes RLPD_RPB transitions.  Wave 0 does the per-row arithmetic (one transition per lane: its R + 3
// rows' gradient values go to LDS) and the block's sums in double, then all four waves write the block's (R + 3) RLPD_RPB gradient
// rows (one non-zero column, the GEMM's K padding zeroed) as 16-byte stores.
template <class P>
__global__ __launch_bounds__(256) void calql_loss_kernel(const CalqlLoss a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  __shared__ float g[(CALQL_MAX_SAMPLES + 3) * RLPD_RPB];  // [j][lane]: j = 0 data, 1 + r random, R + 1 pi, R + 2 pi_next
  const int t = blockIdx.y, R = a.R;
  const int64_t N = a.N, NR = N * R;
  const int64_t row0 = (int64_t)blockIdx.x * RLPD_RPB;
  const float* q = a.q + t * a.q_stride;
  if (threadIdx.x < RLPD_RPB) {
    const int l = threadIdx.x;
    const int64_t n = row0 + l;
    const bool live = n < N;
    const int64_t nn = live ? n : N - 1;
    const float fN = (float)N;
    const float qd = q[nn * a.ldq], y = a.y[nn], ret = a.returns[nn];
    const float qp = q[(N + NR + nn) * a.ldq], qpn = q[(N + NR + N + nn) * a.ldq];
    const float oA = a.per_row ? -a.log_pi[nn] : a.lse[0], oB = a.per_row ? -a.log_pi_next[nn] : a.lse[1];
    const float eA = fmaxf(qp, ret) + oA, eB = fmaxf(qpn, ret) + oB;
    const float* qr = q + (N + nn * R) * a.ldq;
    float mx = fmaxf(eA, eB);
    for (int r = 0; r < R; ++r) mx = fmaxf(mx, qr[(int64_t)r * a.ldq] - a.c);
    float sum = 0.f;
    for (int r = 0; r < R; ++r) {
      const float ex = expf((qr[(int64_t)r * a.ldq] - a.c) - mx);
      g[(1 + r) * RLPD_RPB + l] = ex;
      sum += ex;
    }
    const float xA = expf(eA - mx), xB = expf(eB - mx);
    sum += xA;
    sum += xB;
    const float ood = logf(sum) + mx;
    const float diff = ood - qd;
    const bool pass = diff >= a.clip_min && diff <= a.clip_max;
    const float dcl = fminf(fmaxf(diff, a.clip_min), a.clip_max);
    const float gw = pass ? a.w / fN : 0.f;
    const float d = qd - y;
    const float g0 = (2.f * d) / fN - gw;
    const float gA = (gw * (xA / sum)) * (qp > ret ? 1.f : (qp == ret ? 0.5f : 0.f));
    const float gB = (gw * (xB / sum)) * (qpn > ret ? 1.f : (qpn == ret ? 0.5f : 0.f));
    double s3 = (double)g0;  // the out layer's bias gradient: the sum of the rows before their rounding to elem
    for (int r = 0; r < R; ++r) {
      const float gr = gw * (g[(1 + r) * RLPD_RPB + l] / sum);
      g[(1 + r) * RLPD_RPB + l] = gr;
      s3 += (double)gr;
    }
    s3 += (double)gA;
    s3 += (double)gB;
    g[l] = g0, g[(R + 1) * RLPD_RPB + l] = gA, g[(R + 2) * RLPD_RPB + l] = gB;
    double s0 = live ? (double)(d * d) : 0.0, s1 = live ? (double)qd : 0.0, s2 = live ? (double)y : 0.0, s4 = live ? (double)dcl : 0.0;
    if (!live) s3 = 0.0;
    for (int o = 32; o > 0; o >>= 1) {
      s0 += __shfl_down(s0, o), s1 += __shfl_down(s1, o), s2 += __shfl_down(s2, o), s3 += __shfl_down(s3, o);
      s4 += __shfl_down(s4, o);
    }
    if (threadIdx.x == 0) {
      double* out = a.partial + 4 * ((size_t)t * gridDim.x + blockIdx.x);
      out[0] = s0, out[1] = s1, out[2] = s2, out[3] = s3;
      a.partial_d[(size_t)t * gridDim.x + blockIdx.x] = s4;
    }
  }
  __syncthreads();
  E* dst = (E*)((char*)a.d_out + t * a.d_stride);
  const int cpr = a.ldd / EPC;
  const int rows = (R + 3) * RLPD_RPB;
  for (int i = threadIdx.x; i < rows * cpr; i += 256) {
    const int rr = i / cpr, c = i - rr * cpr;
    int l, j;
    int64_t m;  // the row of the M-row image
    if (rr < RLPD_RPB) {
      l = rr, j = 0, m = row0 + l;
    } else if (rr < (R + 1) * RLPD_RPB) {
      const int u = rr - RLPD_RPB;
      l = u / R, j = 1 + (u - l * R), m = N + (row0 + l) * R + (j - 1);
    } else if (rr < (R + 2) * RLPD_RPB) {
      l = rr - (R + 1) * RLPD_RPB, j = R + 1, m = N + NR + row0 + l;
    } else {
      l = rr - (R + 2) * RLPD_RPB, j = R + 2, m = N + NR + N + row0 + l;
    }
    if (row0 + l >= N) continue;
    union {
      E v[EPC];
      u32x4 u;
    } ch;
#pragma unroll
    for (int k = 0; k < EPC; ++k) ch.v[k] = P::from_f32(0.f);
    if (c == 0) ch.v[0] = P::from_f32(g[j * RLPD_RPB + l]);
    *(u32x4*)(dst + m * a.ldd + c * EPC) = ch.u;
  }
}
// one thread adds the block partials in index order (trunk, then block): no tree to pair them differently
__global__ void calql_finalize_kernel(const double* partial, const double* partial_d, int blocks, int64_t N, float w, double* stats) {
  if (threadIdx.x != 0) return;
  double td[2] = {0.0, 0.0}, df[2] = {0.0, 0.0}, q1 = 0.0, y = 0.0;
  for (int t = 0; t < 2; ++t)
    for (int b = 0; b < blocks; ++b) {
      td[t] += partial[4 * ((size_t)t * blocks + b)];
      df[t] += partial_d[(size_t)t * blocks + b];
    }
  for (int b = 0; b < blocks; ++b) q1 += partial[4 * (size_t)b + 1], y += partial[4 * (size_t)b + 2];
  const double dn = (double)N;
  const double td1 = td[0] / dn, td2 = td[1] / dn, d1 = df[0] / dn, d2 = df[1] / dn;
  stats[0] = ((td1 + td2) + d1 * (double)w) + d2 * (double)w;
  stats[1] = td1 + td2, stats[2] = d1, stats[3] = d2, stats[4] = q1 / dn, stats[5] = y / dn;
}
template <class P>
void launch_calql_loss(const CalqlLoss& a, hipStream_t s) {
  const int blocks = rlpd_blocks(a.N);
  hipLaunchKernelGGL((calql_loss_kernel<P>), dim3(blocks, 2), dim3(256), 0, s, a);
  hipLaunchKernelGGL(calql_finalize_kernel, dim3(1), dim3(64), 0, s, a.partial, a.partial_d, blocks, a.N, a.w, a.stats);
}
template void launch_calql_loss<F32>(const CalqlLoss&, hipStream_t);
template void launch_calql_loss<BF16>(const CalqlLoss&, hipStream_t);

// ---- the actor's choice of the twin and both chains' seeds --------------------------------------------------------------------------
// One wave per row (CALQL_SEL_ROWS rows per block, as ln_rows_kernel): every lane reads the row's two Q values (one cache line each,
// broadcast), so the choice is wave-uniform; lane l then takes the 16-byte chunks l, l + 64, ... of both trunks' rows.  Elementwise:
// an output depends on its own inputs alone and on nothing of the launch geometry.
template <class P>
__global__ __launch_bounds__(256) void calql_select_kernel(const CalqlSelect a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * CALQL_SEL_ROWS + (threadIdx.x >> 6);
  if (n >= a.N) return;  // (wave-uniform)
  const float q1 = a.q1[n * a.ldq], q2 = a.q2[n * a.ldq];
  // (a NaN on either side fails both comparisons: Q1, whose value then reaches the statistics)
  const int sel = q2 < q1 ? 1 : (q1 == q2 ? 2 : 0);
  const float w1 = sel == 0 ? 1.f : (sel == 2 ? 0.5f : 0.f), w2 = sel == 1 ? 1.f : (sel == 2 ? 0.5f : 0.f);
  if (lane == 0) {
    a.sel[n] = (uint8_t)sel;
    a.qsel[n] = sel == 1 ? q2 : q1;
  }
  const int W = a.H / EPC;
  for (int c = lane; c < W; c += 64) {
    CalqlChunk<P> w, x, o;
    w.v = *(const u32x4*)((const E*)a.wout1 + c * EPC);
    x.v = *(const u32x4*)((const E*)a.z1 + n * a.H + c * EPC);
#pragma unroll
    for (int k = 0; k < EPC; ++k) o.e[k] = P::from_f32(w1 == 0.f ? 0.f : w1 * (P::to_f32(w.e[k]) * act_grad_f(a.act, P::to_f32(x.e[k]))));
    *(u32x4*)((E*)a.dz1 + n * a.H + c * EPC) = o.v;
    w.v = *(const u32x4*)((const E*)a.wout2 + c * EPC);
    x.v = *(const u32x4*)((const E*)a.z2 + n * a.H + c * EPC);
#pragma unroll
    for (int k = 0; k < EPC; ++k) o.e[k] = P::from_f32(w2 == 0.f ? 0.f : w2 * (P::to_f32(w.e[k]) * act_grad_f(a.act, P::to_f32(x.e[k]))));
    *(u32x4*)((E*)a.dz2 + n * a.H + c * EPC) = o.v;
  }
}
template <class P>
void launch_calql_select(const CalqlSelect& a, hipStream_t s) {
  if (a.N < 1) return;
  hipLaunchKernelGGL((calql_select_kernel<P>), dim3((unsigned)((a.N + CALQL_SEL_ROWS - 1) / CALQL_SEL_ROWS)), dim3(256), 0, s, a);
}
template void launch_calql_select<F32>(const CalqlSelect&, hipStream_t);
template void launch_calql_select<BF16>(const CalqlSelect&, hipStream_t);

}  // namespace dppo
