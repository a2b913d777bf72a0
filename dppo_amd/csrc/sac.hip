// See sac.h.  gfx950 only.  Compiled with -ffp-contract=off: the head keeps the reference's op sequence (lv = lmin + c (tanh + 1),
// u = mu + sigma z, never an fma; the TD target is idql.hip's, built the same way); the tail's dot product spells its fma out.
#include "sac.h"

namespace dppo {

template <class P>
union SacChunk {
  typename P::elem_t e[16 / P::ESIZE];
  u32x4 v;
};
static unsigned sac_grid(int64_t items) {
  const int64_t blocks = (items + 255) / 256;
  return (unsigned)(blocks > 2048 ? 2048 : (blocks < 1 ? 1 : blocks));
}

// 16 lanes per row: lane `sub` owns elements sub, sub + 16, ...; the row's log-probability is its lanes' partial sums added by
// the xor butterfly, so it depends on that row alone.  The actor call's critic rows [obs | a | 0] are written from the block's
// actions in LDS: one thread per 16-byte chunk.
template <class P>
__global__ __launch_bounds__(256) void sac_head_kernel(const SacHead a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  extern __shared__ float sac_as[];  // [SAC_RPB][AF]
  const dppo_sac_cfg& c = a.cfg;
  const int sub = threadIdx.x & 15, r = threadIdx.x >> 4, AF = a.AF;
  const int64_t row0 = (int64_t)blockIdx.x * SAC_RPB, n = row0 + r, N = a.ring.N;
  float lp = 0.f, sg = 0.f;
  if (n < N) {
    for (int j = sub; j < AF; j += 16) {
      const SacElem e = sac_elem(a, n, j);
      if (a.actions != nullptr) a.actions[n * AF + j] = e.a;
      if (a.u_out != nullptr) a.u_out[n * AF + j] = e.u;
      sac_as[r * AF + j] = e.a;
      const float logsig = c.deterministic ? logf(1e-4f) : 0.5f * e.lv;
      float t = -0.5f * (e.zc * e.zc) - logsig - SAC_LOG_SQRT_2PI;
      if (c.squash) t -= logf(e.s + 1e-6f);
      lp += t;
      sg += e.sigma;
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) lp += __shfl_xor(lp, o), sg += __shfl_xor(sg, o);
  if (n < N && sub == 0) {
    if (a.logp != nullptr) a.logp[n] = lp;
    if (a.sig_row != nullptr) a.sig_row[n] = sg;
  }
  if (a.q1in == nullptr) return;
  __syncthreads();
  const IdqlRows& g = a.ring;
  const int W = a.KpQ / EPC, OD = g.OD;
  for (int i = threadIdx.x; i < SAC_RPB * W; i += 256) {
    const int rr = i / W, cc = i - rr * W;
    const int64_t nn = row0 + rr;
    if (nn >= N) break;
    const float* ob = g.obs + idql_ring_row(g, nn) * OD;
    SacChunk<P> ch;
#pragma unroll
    for (int k = 0; k < EPC; ++k) {
      const int col = cc * EPC + k;
      float x = 0.f;
      if (col < OD)
        x = ob[col];
      else if (col < OD + AF)
        x = sac_as[rr * AF + (col - OD)];
      ch.e[k] = P::from_f32(x);
    }
    *(u32x4*)((E*)a.q1in + nn * a.KpQ + cc * EPC) = ch.v;
    *(u32x4*)((E*)a.q2in + nn * a.KpQ + cc * EPC) = ch.v;
  }
}
template <class P>
void launch_sac_head(const SacHead& a, hipStream_t s) {
  if (a.ring.N < 1) return;
  const unsigned blocks = (unsigned)((a.ring.N + SAC_RPB - 1) / SAC_RPB);
  hipLaunchKernelGGL((sac_head_kernel<P>), dim3(blocks), dim3(256), (size_t)SAC_RPB * a.AF * 4, s, a);
}
template void launch_sac_head<F32>(const SacHead&, hipStream_t);
template void launch_sac_head<BF16>(const SacHead&, hipStream_t);

// ---- the twin's choice and the chains' seeds ------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void sac_select_kernel(const SacSelect a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const int W = a.H / EPC;
  const int64_t total = a.N * 2 * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / (2 * W);
    int c = (int)(i - n * 2 * W);
    const int trunk = c >= W ? 1 : 0;
    if (trunk) c -= W;
    const float q1 = a.q1[n * a.ldq], q2 = a.q2[n * a.ldq];
    const int sel = q2 < q1 ? 1 : 0;
    if (c == 0 && trunk == 0) {
      a.sel[n] = (uint8_t)sel;
      if (a.sel_out != nullptr) a.sel_out[n] = (uint8_t)sel;
      a.qsel[n] = sel ? q2 : q1;
    }
    SacChunk<P> w, x, o;
    w.v = *(const u32x4*)((const E*)(trunk ? a.wout2 : a.wout1) + c * EPC);
    x.v = *(const u32x4*)((const E*)(trunk ? a.z2 : a.z1) + n * a.H + c * EPC);
#pragma unroll
    for (int k = 0; k < EPC; ++k)
      o.e[k] = P::from_f32(sel == trunk ? P::to_f32(w.e[k]) * act_grad_f(a.act, P::to_f32(x.e[k])) : 0.f);
    *(u32x4*)((E*)(trunk ? a.dz2 : a.dz1) + n * a.H + c * EPC) = o.v;
  }
}
template <class P>
void launch_sac_select(const SacSelect& a, hipStream_t s) {
  const int64_t items = a.N * 2 * (a.H / (16 / P::ESIZE));
  if (items < 1) return;
  hipLaunchKernelGGL((sac_select_kernel<P>), dim3(sac_grid(items)), dim3(256), 0, s, a);
}
template void launch_sac_select<F32>(const SacSelect&, hipStream_t);
template void launch_sac_select<BF16>(const SacSelect&, hipStream_t);

// ---- the tail and the head's backward ---------------------------------------------------------------------------------------------
// `rows` rows of dh per block as fp32 in LDS (row stride H2 + 4 floats, as qsm_tail_kernel); thread o of the block's rows * AF
// outputs walks K = 2H in index order with one fma per element: a row's result depends on that row alone.
template <class P>
__global__ __launch_bounds__(256) void sac_tail_kernel(const SacTail a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  extern __shared__ float sac_xs[];
  const SacHead& hd = a.head;
  const int H2 = a.H2, LD = H2 + 4, AF = hd.AF, cpr = H2 / EPC;
  const int64_t N = hd.ring.N, row0 = (int64_t)blockIdx.x * a.rows;
  for (int i = threadIdx.x; i < a.rows * cpr; i += 256) {
    const int r = i / cpr, c = i - r * cpr;
    SacChunk<P> ch;
    if (row0 + r < N)
      ch.v = *(const u32x4*)((const E*)a.dh + (row0 + r) * H2 + c * EPC);
    else
      ch.v = u32x4{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < EPC; ++k) sac_xs[r * LD + c * EPC + k] = P::to_f32(ch.e[k]);
  }
  const int pad = a.ldd - 2 * AF;  // the K padding of the backward's first GEMM
  for (int i = threadIdx.x; i < a.rows * pad; i += 256) {
    const int r = i / pad, c = i - r * pad;
    if (row0 + r < N) ((E*)a.d_out)[(row0 + r) * a.ldd + 2 * AF + c] = P::from_f32(0.f);
  }
  __syncthreads();
  const float alpha = (float)*a.alpha, fN = (float)N;
  for (int o = threadIdx.x; o < a.rows * AF; o += 256) {
    const int r = o / AF, j = o - r * AF;
    const int64_t n = row0 + r;
    if (n >= N) break;
    const float* x = sac_xs + r * LD;
    const E* w = (const E*)a.wa + (int64_t)j * H2;
    float acc = 0.f;
    for (int k = 0; k < H2; k += EPC) {
      SacChunk<P> wc;
      wc.v = *(const u32x4*)(w + k);
#pragma unroll
      for (int e = 0; e < EPC; e += 4) {
        const f32x4 xv = *(const f32x4*)(x + k + e);
        acc = __builtin_fmaf(xv.x, P::to_f32(wc.e[e]), acc);
        acc = __builtin_fmaf(xv.y, P::to_f32(wc.e[e + 1]), acc);
        acc = __builtin_fmaf(xv.z, P::to_f32(wc.e[e + 2]), acc);
        acc = __builtin_fmaf(xv.w, P::to_f32(wc.e[e + 3]), acc);
      }
    }
    const SacElem e = sac_elem(hd, n, j);
    float du = -(acc * e.s);
    if (hd.cfg.squash) {
      const float t0 = (alpha * 2.f) * (e.a * e.s);
      du = du + t0 / (e.s + 1e-6f);
    }
    du = du / fN;
    const float t1 = du * e.zc;
    const float dsig = t1 - alpha / (fN * e.sigma);
    const float t2 = dsig * (0.5f * e.sigma);
    const float draw = t2 * (hd.half_span * sac_sech2(e.raw));
    ((E*)a.d_out)[n * a.ldd + j] = P::from_f32(du);
    ((E*)a.d_out)[n * a.ldd + AF + j] = P::from_f32(draw);
    if (a.d_out32 != nullptr) a.d_out32[n * 2 * AF + j] = du, a.d_out32[n * 2 * AF + AF + j] = draw;
    if (a.d_a != nullptr) a.d_a[n * AF + j] = -acc / fN;
  }
}
template <class P>
void launch_sac_tail(const SacTail& a, hipStream_t s) {
  if (a.head.ring.N < 1 || a.rows < 1) return;
  const unsigned blocks = (unsigned)((a.head.ring.N + a.rows - 1) / a.rows);
  hipLaunchKernelGGL((sac_tail_kernel<P>), dim3(blocks), dim3(256), (size_t)a.rows * (a.H2 + 4) * 4, s, a);
}
template void launch_sac_tail<F32>(const SacTail&, hipStream_t);
template void launch_sac_tail<BF16>(const SacTail&, hipStream_t);

// ---- fixed-order sums ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sac_stats_kernel(const SacStats a) {
  __shared__ double sh[4][256];
  const float alpha = (float)*a.alpha;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t n = threadIdx.x; n < a.N; n += 256) {
    const float q = a.qsel[n], lp = a.logp[n];
    const float t = alpha * lp;
    v[0] += (double)(-q + t), v[1] += q, v[2] += lp, v[3] += a.sig_row[n];
  }
  sac_tree<4>(sh, v);
  if (threadIdx.x == 0) {
    const double dn = (double)a.N;
    a.stats[0] = sh[0][0] / dn, a.stats[1] = sh[1][0] / dn, a.stats[2] = sh[2][0] / dn, a.stats[3] = sh[3][0] / (dn * a.AF);
  }
}
void launch_sac_stats(const SacStats& a, hipStream_t s) { hipLaunchKernelGGL(sac_stats_kernel, dim3(1), dim3(256), 0, s, a); }

__global__ __launch_bounds__(256) void sac_alpha_kernel(const float* logp, int64_t N, const double* log_alpha, double te, double* out) {
  __shared__ double sh[1][256];
  double v[1] = {0.0};
  for (int64_t n = threadIdx.x; n < N; n += 256) v[0] += logp[n];
  sac_tree<1>(sh, v);
  if (threadIdx.x == 0) {
    const double loss = -exp(*log_alpha) * (sh[0][0] / (double)N + te);
    out[0] = loss, out[1] = loss;
  }
}
void launch_sac_alpha_loss(const float* logp, int64_t N, const double* log_alpha, double target_entropy, double* out, hipStream_t s) {
  hipLaunchKernelGGL(sac_alpha_kernel, dim3(1), dim3(256), 0, s, logp, N, log_alpha, target_entropy, out);
}

}  // namespace dppo
