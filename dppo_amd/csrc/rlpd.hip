// See rlpd.h.  gfx950 only.  Compiled with -ffp-contract=off: the statistics keep torch's op sequence (two-pass, biased
// variance, separate products and sums).
#include "rlpd.h"

namespace dppo {

__device__ __forceinline__ float wave_sum64(float x) {  // xor butterfly: every lane ends with the same total
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// One wave per row; lane l owns the 4 consecutive features 4 l + 256 k.  The row is read three times (mean, variance, output):
// it is at most a few KB and stays in L1.
template <class P>
__global__ __launch_bounds__(256) void ln_rows_kernel(const LnRows a) {
  typedef typename P::elem_t E;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * LN_ROWS_PB + (threadIdx.x >> 6);
  if (row >= a.M) return;  // (wave-uniform)
  const float* x = a.x + row * a.ldx;
  float s = 0.f;
  for (int c = 4 * lane; c < a.H; c += 256) {
    const float4 v = *(const float4*)(x + c);
    s += (v.x + v.y) + (v.z + v.w);
  }
  const float inv = 1.f / (float)a.H;
  const float mean = wave_sum64(s) * inv;
  float q = 0.f;
  for (int c = 4 * lane; c < a.H; c += 256) {
    const float4 v = *(const float4*)(x + c);
    const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float rstd = 1.f / sqrtf(wave_sum64(q) * inv + PLAIN_LN_EPS);
  if (a.stats != nullptr && lane == 0) a.stats[2 * row] = mean, a.stats[2 * row + 1] = rstd;
  with_act(a.act, [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    for (int c = 4 * lane; c < a.H; c += 256) {
      const float4 v = *(const float4*)(x + c);
      const float xv[4] = {v.x, v.y, v.z, v.w};
      float z[4], w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        z[e] = (xv[e] - mean) * rstd * a.gamma[c + e] + a.beta[c + e];
        w[e] = act_c<ACT>(z[e]);
      }
      E* oa = (E*)a.out_act + row * a.ldo + c;
      E* oz = a.out_z != nullptr ? (E*)a.out_z + row * a.ldo + c : nullptr;
      if constexpr (P::ESIZE == 4) {
        *(float4*)oa = make_float4(w[0], w[1], w[2], w[3]);
        if (oz != nullptr) *(float4*)oz = make_float4(z[0], z[1], z[2], z[3]);
      } else {
        u32x2 pk;
        pk.x = (uint32_t)f2bf(w[0]) | ((uint32_t)f2bf(w[1]) << 16);
        pk.y = (uint32_t)f2bf(w[2]) | ((uint32_t)f2bf(w[3]) << 16);
        *(u32x2*)oa = pk;
        if (oz != nullptr) {
          pk.x = (uint32_t)f2bf(z[0]) | ((uint32_t)f2bf(z[1]) << 16);
          pk.y = (uint32_t)f2bf(z[2]) | ((uint32_t)f2bf(z[3]) << 16);
          *(u32x2*)oz = pk;
        }
      }
    }
  });
}
template <class P>
void launch_ln_rows(const LnRows& a, hipStream_t s) {
  if (a.M < 1) return;
  hipLaunchKernelGGL((ln_rows_kernel<P>), dim3((unsigned)((a.M + LN_ROWS_PB - 1) / LN_ROWS_PB)), dim3(256), 0, s, a);
}
template void launch_ln_rows<F32>(const LnRows&, hipStream_t);
template void launch_ln_rows<BF16>(const LnRows&, hipStream_t);


// ---- LayerNorm backward -------------------------------------------------------------------------------------------------------
int ln_bwd_blocks(int64_t M) { return (int)((M + LN_BWD_ROWS - 1) / LN_BWD_ROWS); }

// Wave w of a block takes rows row0 + w, row0 + w + 4, ...; lane l owns columns 4 l + 256 k, k < 4 (H <= LN_MAX_H).
template <class P>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnBwd a) {
  typedef typename P::elem_t E;
  constexpr int KM = LN_MAX_H / 256;
  __shared__ float red[4][2][LN_MAX_H];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * LN_BWD_ROWS;
  const float inv = 1.f / (float)a.H;
  float dg[KM][4], db[KM][4], ga[KM][4];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int c = 4 * lane + 256 * k;
#pragma unroll
    for (int e = 0; e < 4; ++e) dg[k][e] = db[k][e] = 0.f, ga[k][e] = c < a.H ? a.gamma[c + e] : 0.f;
  }
  for (int i = 0; i < LN_BWD_ROWS / 4; ++i) {
    const int64_t row = row0 + w + 4 * i;
    if (row >= a.M) break;  // (wave-uniform)
    const float mean = a.stats[2 * row], rstd = a.stats[2 * row + 1];
    float g[KM][4], xh[KM][4];
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int c = 4 * lane + 256 * k;
      if (c < a.H) {
        float dz[4];
        if (a.dz32 != nullptr) {  // (kernel-uniform)
          const float4 t = *(const float4*)(a.dz32 + row * a.ld + c);
          dz[0] = t.x, dz[1] = t.y, dz[2] = t.z, dz[3] = t.w;
        } else {
          load4<P>((const E*)a.dz + row * a.ld + c, dz);
        }
        const float4 xv = *(const float4*)(a.x + row * a.ldx + c);
        const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xh[k][e] = (x4[e] - mean) * rstd;
          dg[k][e] += dz[e] * xh[k][e];
          db[k][e] += dz[e];
          g[k][e] = ga[k][e] * dz[e];
          s0 += g[k][e];
          s1 += g[k][e] * xh[k][e];
        }
      }
    }
    s0 = wave_sum64(s0) * inv, s1 = wave_sum64(s1) * inv;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int c = 4 * lane + 256 * k;
      if (c < a.H) {
        float dx[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) dx[e] = rstd * (g[k][e] - s0 - xh[k][e] * s1);
        store4<P>((E*)a.dz + row * a.ld + c, dx);
      }
    }
  }
  if (a.partial == nullptr) return;  // (block-uniform)
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < a.H) {
#pragma unroll
      for (int e = 0; e < 4; ++e) red[w][0][c + e] = dg[k][e], red[w][1][c + e] = db[k][e];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * a.H; i += 256) {
    const int which = i / a.H, c = i - which * a.H;
    a.partial[((size_t)blockIdx.x * 2 + which) * a.H + c] = ((red[0][which][c] + red[1][which][c]) + red[2][which][c]) + red[3][which][c];
  }
}
// the block partials are added in index order by one thread per column
__global__ __launch_bounds__(256) void ln_bwd_finalize_kernel(const float* partial, int blocks, int H, float* dgamma, float* dbeta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * H) return;
  const int which = i / H, c = i - which * H;
  float s = 0.f;
  for (int b = 0; b < blocks; ++b) s += partial[((size_t)b * 2 + which) * H + c];
  (which ? dbeta : dgamma)[c] = s;
}
template <class P>
void launch_ln_bwd(const LnBwd& a, hipStream_t s) {
  if (a.M < 1) return;
  const int blocks = ln_bwd_blocks(a.M);
  hipLaunchKernelGGL((ln_bwd_kernel<P>), dim3(blocks), dim3(256), 0, s, a);
  if (a.partial != nullptr)
    hipLaunchKernelGGL(ln_bwd_finalize_kernel, dim3((2 * a.H + 255) / 256), dim3(256), 0, s, a.partial, blocks, a.H, a.dgamma, a.dbeta);
}
template void launch_ln_bwd<F32>(const LnBwd&, hipStream_t);
template void launch_ln_bwd<BF16>(const LnBwd&, hipStream_t);

// ---- the ensemble's TD loss (gaussian_rlpd.py:64-103) ----------------------------------------------------------------------------
// blockIdx.y is the member.  Wave 0 does the per-row arithmetic (one row per lane) and the block's three sums in double, then all
// four waves write the gradient rows (one non-zero column, the GEMM's K padding zeroed) as 16-byte stores.
int rlpd_blocks(int64_t N) { return (int)((N + RLPD_RPB - 1) / RLPD_RPB); }
template <class P>
__global__ __launch_bounds__(256) void rlpd_loss_kernel(const RlpdLoss a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  __shared__ float g[RLPD_RPB];
  const int e = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.x * RLPD_RPB;
  if (threadIdx.x < RLPD_RPB) {
    const int64_t n = row0 + threadIdx.x;
    const bool live = n < a.N;
    const int64_t nn = live ? n : a.N - 1;
    const float m = a.gamma * (1.f - a.terminated[nn]);
    const float nq = fminf(a.t1[nn * a.ldt], a.t2[nn * a.ldt]);
    float y = a.reward[nn] + m * nq;
    if (a.next_logp != nullptr) y = y + (m * (float)*a.alpha) * (-a.next_logp[nn]);
    const float q = a.q[e * a.q_stride + nn * a.ldq];
    const float d = q - y;
    g[threadIdx.x] = (2.f * d) / (float)((int64_t)a.E * a.N);
    double s0 = live ? (double)(d * d) : 0.0, s1 = live ? (double)q : 0.0, s2 = live ? (double)y : 0.0;
    double s3 = live ? (double)g[threadIdx.x] : 0.0;  // the out layer's bias gradient, from the rows before their rounding to elem
    for (int o = 32; o > 0; o >>= 1)
      s0 += __shfl_down(s0, o), s1 += __shfl_down(s1, o), s2 += __shfl_down(s2, o), s3 += __shfl_down(s3, o);
    if (threadIdx.x == 0) {
      double* out = a.partial + 4 * ((size_t)e * gridDim.x + blockIdx.x);
      out[0] = s0, out[1] = s1, out[2] = s2, out[3] = s3;
    }
  }
  __syncthreads();
  E* dst = (E*)((char*)a.d_out + e * a.d_stride);
  const int cpr = a.ldd / EPC;
  for (int i = threadIdx.x; i < RLPD_RPB * cpr; i += 256) {
    const int r = i / cpr, c = i - r * cpr;
    if (row0 + r >= a.N) break;
    union {
      E v[EPC];
      u32x4 u;
    } ch;
#pragma unroll
    for (int k = 0; k < EPC; ++k) ch.v[k] = P::from_f32(0.f);
    if (c == 0) ch.v[0] = P::from_f32(g[r]);
    *(u32x4*)(dst + (row0 + r) * a.ldd + c * EPC) = ch.u;
  }
}
// one lane per statistic adds the block partials in index order (member, then block): no tree to pair them differently
__global__ void rlpd_finalize_kernel(const double* partial, int blocks, int E, int64_t N, double* stats) {
  if (threadIdx.x >= 3) return;
  double s = 0;
  const int members = threadIdx.x == 2 ? 1 : E;  // y is the same for every member
  for (int i = 0; i < members * blocks; ++i) s += partial[4 * (size_t)i + threadIdx.x];
  stats[threadIdx.x] = s / ((double)members * (double)N);
}
// member e's d loss / d bout = sum_n of its gradient rows, the block partials added in index order
__global__ void rlpd_out_bias_kernel(const double* partial, int blocks, int E, float* grad, int64_t stride, int64_t bout) {
  const int e = threadIdx.x;
  if (e >= E) return;
  double s = 0;
  for (int b = 0; b < blocks; ++b) s += partial[4 * ((size_t)e * blocks + b) + 3];
  grad[e * stride + bout] = (float)s;
}
void launch_rlpd_out_bias(const double* partial, int64_t N, int E, float* grad, int64_t stride, int64_t bout, hipStream_t s) {
  hipLaunchKernelGGL(rlpd_out_bias_kernel, dim3(1), dim3(64), 0, s, partial, rlpd_blocks(N), E, grad, stride, bout);
}
template <class P>
void launch_rlpd_loss(const RlpdLoss& a, hipStream_t s) {
  const int blocks = rlpd_blocks(a.N);
  hipLaunchKernelGGL((rlpd_loss_kernel<P>), dim3(blocks, a.E), dim3(256), 0, s, a);
  hipLaunchKernelGGL(rlpd_finalize_kernel, dim3(1), dim3(64), 0, s, a.partial, blocks, a.E, a.N, a.stats);
}
template void launch_rlpd_loss<F32>(const RlpdLoss&, hipStream_t);
template void launch_rlpd_loss<BF16>(const RlpdLoss&, hipStream_t);

// ---- the actor's loss through the ensemble's mean (gaussian_rlpd.py:100-112) ------------------------------------------------------
// 16 outputs per block, 16 lanes per output; every lane of a wave runs the product (an output past the end redoes the last one and
// writes nothing), so the butterfly never meets an idle lane.  Lane 0 of an output then runs the head's backward.
template <class P>
__global__ __launch_bounds__(256) void rlpd_tail_kernel(const RlpdTail a) {
  typedef typename P::elem_t E;
  const SacHead& hd = a.head;
  const int AF = hd.AF, sub = threadIdx.x & (RLPD_TAIL_LANES - 1);
  const int64_t N = hd.ring.N, total = N * AF;
  const int64_t o = (int64_t)blockIdx.x * (256 / RLPD_TAIL_LANES) + (threadIdx.x / RLPD_TAIL_LANES);
  const bool live = o < total;
  const int64_t oo = live ? o : total - 1;
  const int64_t n = oo / AF;
  const int j = (int)(oo - n * AF);
  const E* x = (const E*)a.dh + n * a.K;
  const E* w = (const E*)a.wa + (int64_t)j * a.K;
  float acc = 0.f;
  for (int k = 4 * sub; k < a.K; k += 4 * RLPD_TAIL_LANES) {
    float xv[4], wv[4];
    load4<P>(x + k, xv);
    load4<P>(w + k, wv);
    acc = __builtin_fmaf(xv[0], wv[0], acc);
    acc = __builtin_fmaf(xv[1], wv[1], acc);
    acc = __builtin_fmaf(xv[2], wv[2], acc);
    acc = __builtin_fmaf(xv[3], wv[3], acc);
  }
#pragma unroll
  for (int m = 1; m < RLPD_TAIL_LANES; m <<= 1) acc += __shfl_xor(acc, m);
  if (!live) return;
  if (j == 0) {  // the K padding of the backward's first GEMM
    const int pad = a.ldd - 2 * AF;
    for (int c = sub; c < pad; c += RLPD_TAIL_LANES) ((E*)a.d_out)[n * a.ldd + 2 * AF + c] = P::from_f32(0.f);
  }
  if (sub != 0) return;
  const float g = acc / (float)a.E;  // the members' mean: 1/E once, behind the whole sum
  const float alpha = (float)*a.alpha, fN = (float)N;
  const SacElem e = sac_elem(hd, n, j);
  float du = -(g * e.s);
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
  if (a.d_a != nullptr) a.d_a[n * AF + j] = -g / fN;
}
template <class P>
void launch_rlpd_tail(const RlpdTail& a, hipStream_t s) {
  const int64_t total = a.head.ring.N * a.head.AF;
  if (total < 1) return;
  constexpr int OPB = 256 / RLPD_TAIL_LANES;
  hipLaunchKernelGGL((rlpd_tail_kernel<P>), dim3((unsigned)((total + OPB - 1) / OPB)), dim3(256), 0, s, a);
}
template void launch_rlpd_tail<F32>(const RlpdTail&, hipStream_t);
template void launch_rlpd_tail<BF16>(const RlpdTail&, hipStream_t);

__global__ __launch_bounds__(256) void rlpd_actor_stats_kernel(const RlpdActorStats a) {
  __shared__ double sh[4][256];
  const float alpha = (float)*a.alpha;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t n = threadIdx.x; n < a.N; n += 256) {
    float q = 0.f;
    for (int e = 0; e < a.E; ++e) q += a.q[e * a.q_stride + n * a.ldq];
    q = q / (float)a.E;
    const float lp = a.logp[n];
    const float t = alpha * lp;
    v[0] += (double)(-q + t), v[1] += q, v[2] += lp, v[3] += a.sig_row[n];
  }
  sac_tree<4>(sh, v);
  if (threadIdx.x == 0) {
    const double dn = (double)a.N;
    a.stats[0] = sh[0][0] / dn, a.stats[1] = sh[1][0] / dn, a.stats[2] = sh[2][0] / dn, a.stats[3] = sh[3][0] / (dn * a.AF);
  }
}
void launch_rlpd_actor_stats(const RlpdActorStats& a, hipStream_t s) {
  hipLaunchKernelGGL(rlpd_actor_stats_kernel, dim3(1), dim3(256), 0, s, a);
}

}  // namespace dppo
