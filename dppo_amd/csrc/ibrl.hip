// See ibrl.h.  gfx950 only.  Compiled with -ffp-contract=off: every product and sum below is torch's, none is fused.
#include "ibrl.h"

namespace dppo {

// torch.min(a, b): a NaN on either side is the result (fminf would drop it)
__device__ __forceinline__ float ibrl_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// ---- dropout behind a plain hidden layer ----------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void drop_rows_kernel(const DropRows a) {
  typedef typename P::elem_t E;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * LN_ROWS_PB + (threadIdx.x >> 6);
  if (row >= a.M) return;  // (wave-uniform)
  const float* x = a.x + row * a.ldx;
  const int64_t m0 = ((int64_t)a.layer * a.M + row) * a.H;  // this row's place in the mask's [L][M][H]
  with_act(a.act, [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    for (int c = 4 * lane; c < a.H; c += 256) {
      const float4 v = *(const float4*)(x + c);
      const float xv[4] = {v.x, v.y, v.z, v.w};
      uint32_t kw = 0;  // byte e: keep of feature c + e
      if (a.mask != nullptr) {
        kw = *(const uint32_t*)(a.mask + m0 + c);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          uint32_t c0, c1;
          philox4x32_10((uint64_t)(m0 + c + e), a.k0, a.k1, c0, c1);
          const float u = (float)(c0 >> 8) * 5.9604644775390625e-08f;  // 2^-24: [0, 1), exact
          kw |= (u >= a.p ? 1u : 0u) << (8 * e);
        }
      }
      if (a.mask_out != nullptr) *(uint32_t*)(a.mask_out + m0 + c) = kw & 0x01010101u;
      float z[4], w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        z[e] = ((kw >> (8 * e)) & 0xffu) != 0 ? xv[e] * a.scale : 0.f;
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
void launch_drop_rows(const DropRows& a, hipStream_t s) {
  if (a.M < 1) return;
  hipLaunchKernelGGL((drop_rows_kernel<P>), dim3((unsigned)((a.M + LN_ROWS_PB - 1) / LN_ROWS_PB)), dim3(256), 0, s, a);
}
template void launch_drop_rows<F32>(const DropRows&, hipStream_t);
template void launch_drop_rows<BF16>(const DropRows&, hipStream_t);

// ---- row builder ------------------------------------------------------------------------------------------------------------------
// One thread per 16-byte chunk of a row's operand image; sections of a row n: 0 the members' row (with qin), 1 the BC target row, 2
// the RL target row.
template <class P>
__global__ __launch_bounds__(256) void ibrl_rows_kernel(const IbrlRows a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const IdqlRows& g = a.ring;
  const int W = a.Kp / EPC, OD = g.OD, AD = g.AD;
  const int first = a.qin != nullptr ? 0 : 1, SW = (3 - first) * W;
  const int64_t total = g.N * SW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / SW;
    int c = (int)(i - n * SW);
    const int sec = first + c / W;
    c -= (sec - first) * W;
    const int64_t row = idql_ring_row(g, n);
    if (c == 0 && sec == 0 && a.r_out != nullptr) {
      a.r_out[n] = g.reward[row];
      a.term_out[n] = g.terminated[row];
    }
    const float* ob = (sec == 0 ? g.obs : g.next_obs) + row * OD;
    const float* ac = sec == 0 ? g.actions + row * AD : (sec == 1 ? a.a_bc : a.a_rl) + n * AD;
    union {
      E e[EPC];
      u32x4 v;
    } ch;
#pragma unroll
    for (int k = 0; k < EPC; ++k) {
      const int col = c * EPC + k;
      float x = 0.f;
      if (col < OD)
        x = ob[col];
      else if (col < OD + AD)
        x = ac[col - OD];
      ch.e[k] = P::from_f32(x);
    }
    E* dst = sec == 0 ? (E*)a.qin + n * a.Kp : (E*)a.tin + (n + (sec == 2 ? g.N : 0)) * a.Kp;
    *(u32x4*)(dst + c * EPC) = ch.v;
  }
}
template <class P>
void launch_ibrl_rows(const IbrlRows& a, hipStream_t s) {
  const int64_t items = a.ring.N * (a.qin != nullptr ? 3 : 2) * (a.Kp / (16 / P::ESIZE));
  if (items < 1) return;
  const int64_t blocks = (items + 255) / 256;
  hipLaunchKernelGGL((ibrl_rows_kernel<P>), dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, s, a);
}
template void launch_ibrl_rows<F32>(const IbrlRows&, hipStream_t);
template void launch_ibrl_rows<BF16>(const IbrlRows&, hipStream_t);

// ---- the TD target's bootstrap value ------------------------------------------------------------------------------------------------
int ibrl_target_blocks(int64_t N) { return (int)((N + 255) / 256); }
// the block's count: per wave by shuffles, the four waves through LDS in wave order; ibrl_share_kernel adds the blocks in index order
__global__ __launch_bounds__(256) void ibrl_target_kernel(const IbrlTarget a) {
  __shared__ uint32_t cnt[4];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t won = 0;
  if (n < a.N) {
    const float mb = ibrl_min(a.t1[n * a.ldt], a.t2[n * a.ldt]);
    const float mr = ibrl_min(a.t1[(a.N + n) * a.ldt], a.t2[(a.N + n) * a.ldt]);
    won = mb > mr ? 1u : 0u;
    const float tq = won ? mb : mr;
    a.tq[n] = tq;
    if (a.y_out != nullptr) a.y_out[n] = a.reward[n] + (a.gamma * (1.f - a.terminated[n])) * tq;
  }
  for (int o = 32; o > 0; o >>= 1) won += __shfl_down(won, o);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = won;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[blockIdx.x] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}
__global__ void ibrl_share_kernel(const uint32_t* partial, int blocks, int64_t N, double* share) {
  uint64_t s = 0;
  for (int b = 0; b < blocks; ++b) s += partial[b];
  *share = (double)s / (double)N;
}
void launch_ibrl_target(const IbrlTarget& a, hipStream_t s) {
  const int blocks = ibrl_target_blocks(a.N);
  hipLaunchKernelGGL(ibrl_target_kernel, dim3(blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(ibrl_share_kernel, dim3(1), dim3(1), 0, s, a.partial, blocks, a.N, a.share);
}

// ---- Q-guided choice between the two proposals ----------------------------------------------------------------------------------------
// One thread per action element; every thread of a row redoes the row's decision (two exponentials), element 0 writes the row's outputs.
__global__ __launch_bounds__(256) void ibrl_select_kernel(const IbrlSelect a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N * a.AF) return;
  const int64_t n = i / a.AF;
  const float qb = ibrl_min(a.q1[n * a.ldq], a.q2[n * a.ldq]);
  const float qr = ibrl_min(a.q1[(a.N + n) * a.ldq], a.q2[(a.N + n) * a.ldq]);
  bool bc = qb > qr;
  if (a.soft) {
    const float wb = expf(qb * a.beta), wr = expf(qr * a.beta);
    const float d = wr - wb;
    if (d == d) {
      const float pb = 1.f / (1.f + expf(d));
      float u;
      if (a.u != nullptr) {
        u = a.u[n];
      } else {
        uint32_t c0, c1;
        philox4x32_10((uint64_t)n, a.k0, a.k1, c0, c1);
        u = (float)(c0 >> 8) * 5.9604644775390625e-08f;
      }
      bc = u < pb;
    }
  }
  a.action[i] = bc ? a.a_bc[i] : a.a_rl[i];
  if (i == n * a.AF) {
    a.q_bc[n] = qb, a.q_rl[n] = qr;
    a.took_bc[n] = bc ? 1 : 0;
  }
}
void launch_ibrl_select(const IbrlSelect& a, hipStream_t s) {
  const int64_t tot = a.N * a.AF;
  hipLaunchKernelGGL(ibrl_select_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
}

// ---- the actor's loss through the ensemble's min (gaussian_ibrl.py:115-128) ---------------------------------------------------------
template <class P>
union IbrlChunk {
  typename P::elem_t e[16 / P::ESIZE];
  u32x4 v;
};

// The backward of drop_rows_kernel's z' = keep ? z s : 0, with its geometry: one wave per row, lane l owns features 4 l + 256 k.
template <class P>
__global__ __launch_bounds__(256) void drop_bwd_kernel(const DropBwd a) {
  typedef typename P::elem_t E;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * LN_ROWS_PB + (threadIdx.x >> 6);
  if (row >= a.M) return;  // (wave-uniform)
  const int64_t m0 = ((int64_t)a.layer * a.M + row) * a.H;
  E* dz = (E*)a.dz + row * a.ld;
  for (int c = 4 * lane; c < a.H; c += 256) {
    float g[4];
    load4<P>(dz + c, g);
    const uint32_t kw = *(const uint32_t*)(a.mask + m0 + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = ((kw >> (8 * e)) & 0xffu) != 0 ? g[e] * a.scale : 0.f;
    store4<P>(dz + c, g);
  }
}
template <class P>
void launch_drop_bwd(const DropBwd& a, hipStream_t s) {
  if (a.M < 1) return;
  hipLaunchKernelGGL((drop_bwd_kernel<P>), dim3((unsigned)((a.M + LN_ROWS_PB - 1) / LN_ROWS_PB)), dim3(256), 0, s, a);
}
template void launch_drop_bwd<F32>(const DropBwd&, hipStream_t);
template void launch_drop_bwd<BF16>(const DropBwd&, hipStream_t);

// The head.  An action column belongs to exactly one chunk of the row image, so its thread is the one that forms and stores it.
template <class P>
__global__ __launch_bounds__(256) void ibrl_head_kernel(const IbrlHead a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const IdqlRows& g = a.ring;
  const dppo_gaussian_cfg& cf = a.cfg;
  const int W = a.Kp / EPC, OD = g.OD, AF = g.AD;
  const int64_t total = g.N * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / W;
    const int c = (int)(i - n * W);
    const float* ob = g.obs + idql_ring_row(g, n) * OD;
    IbrlChunk<P> ch;
#pragma unroll
    for (int k = 0; k < EPC; ++k) {
      const int col = c * EPC + k;
      float x = 0.f;
      if (col < OD) {
        x = ob[col];
      } else if (col < OD + AF) {
        const int j = col - OD;
        const int64_t el = n * AF + j;
        const float m = a.out[n * a.ldo + j];
        const float mu = cf.tanh_mean ? tanhf(m) : m;
        float z = a.noise != nullptr ? a.noise[el] : philox_normal((uint64_t)el, cf.seed_lo, cf.seed_hi);
        z = fminf(fmaxf(z, -cf.randn_clip), cf.randn_clip);
        x = mu + cf.fixed_std * z;  // (gauss_sample_kernel's arithmetic)
        a.actions[el] = x;
        a.mu[el] = mu;
      }
      ch.e[k] = P::from_f32(x);
    }
    *(u32x4*)((E*)a.qin + n * a.Kp + c * EPC) = ch.v;
  }
}
template <class P>
void launch_ibrl_head(const IbrlHead& a, hipStream_t s) {
  const int64_t items = a.ring.N * (a.Kp / (16 / P::ESIZE));
  if (items < 1) return;
  const int64_t blocks = (items + 255) / 256;
  hipLaunchKernelGGL((ibrl_head_kernel<P>), dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, s, a);
}
template void launch_ibrl_head<F32>(const IbrlHead&, hipStream_t);
template void launch_ibrl_head<BF16>(const IbrlHead&, hipStream_t);

// The min over the members and the chains' seeds.  One wave per row: every lane reads the row's E values (broadcast loads), so the
// choice is wave-uniform; lane l then takes the 16-byte chunks l, l + 64, ... of every member's row.
template <class P>
__global__ __launch_bounds__(256) void ibrl_min_kernel(const IbrlMin a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * LN_ROWS_PB + (threadIdx.x >> 6);
  if (n >= a.N) return;  // (wave-uniform)
  float best = a.q[n * a.ldq];
  int sel = 0;
  for (int e = 1; e < a.E; ++e) {
    const float q = a.q[e * a.q_stride + n * a.ldq];
    // torch.min along a dimension: the first NaN stays; otherwise strictly smaller moves, so a tie keeps the lowest index
    if (best == best && (q != q || q < best)) best = q, sel = e;
  }
  if (lane == 0) {
    a.qmin[n] = best;
    a.sel[n] = (uint8_t)sel;
  }
  const int W = a.H / EPC;
  for (int e = 0; e < a.E; ++e) {
    E* out = (E*)a.dz[e] + n * a.H;
    if (e != sel) {
      u32x4 zero;
      zero.x = zero.y = zero.z = zero.w = 0u;
      for (int c = lane; c < W; c += 64) *(u32x4*)(out + c * EPC) = zero;
      continue;
    }
    const E* wo = (const E*)a.wout[e];
    const E* zr = (const E*)a.z[e] + n * a.H;
    for (int c = lane; c < W; c += 64) {
      IbrlChunk<P> w, x, o;
      w.v = *(const u32x4*)(wo + c * EPC);
      x.v = *(const u32x4*)(zr + c * EPC);
#pragma unroll
      for (int k = 0; k < EPC; ++k) o.e[k] = P::from_f32(P::to_f32(w.e[k]) * act_grad_f(a.act, P::to_f32(x.e[k])));
      *(u32x4*)(out + c * EPC) = o.v;
    }
  }
}
template <class P>
void launch_ibrl_min(const IbrlMin& a, hipStream_t s) {
  if (a.N < 1) return;
  hipLaunchKernelGGL((ibrl_min_kernel<P>), dim3((unsigned)((a.N + LN_ROWS_PB - 1) / LN_ROWS_PB)), dim3(256), 0, s, a);
}
template void launch_ibrl_min<F32>(const IbrlMin&, hipStream_t);
template void launch_ibrl_min<BF16>(const IbrlMin&, hipStream_t);

// The chains' tail and the head's backward: rlpd_tail_kernel's product (16 outputs per block, 16 lanes per output, every lane of a
// wave runs the product, an output past the end redoes the last one and writes nothing), then the fixed-std head.
template <class P>
__global__ __launch_bounds__(256) void ibrl_tail_kernel(const IbrlTail a) {
  typedef typename P::elem_t E;
  const int AF = a.AF, sub = threadIdx.x & (RLPD_TAIL_LANES - 1);
  const int64_t total = a.N * AF;
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
    const int pad = a.ldd - AF;
    for (int c = sub; c < pad; c += RLPD_TAIL_LANES) ((E*)a.d_out)[n * a.ldd + AF + c] = P::from_f32(0.f);
  }
  if (sub != 0) return;
  const float da = -acc / (float)a.N;
  float du = da;
  if (a.tanh_mean) {
    const float mu = a.mu[n * AF + j];
    du = da * (1.f - mu * mu);
  }
  ((E*)a.d_out)[n * a.ldd + j] = P::from_f32(du);
  if (a.d_out32 != nullptr) a.d_out32[n * AF + j] = du;
  if (a.d_a != nullptr) a.d_a[n * AF + j] = da;
}
template <class P>
void launch_ibrl_tail(const IbrlTail& a, hipStream_t s) {
  const int64_t total = a.N * a.AF;
  if (total < 1) return;
  constexpr int OPB = 256 / RLPD_TAIL_LANES;
  hipLaunchKernelGGL((ibrl_tail_kernel<P>), dim3((unsigned)((total + OPB - 1) / OPB)), dim3(256), 0, s, a);
}
template void launch_ibrl_tail<F32>(const IbrlTail&, hipStream_t);
template void launch_ibrl_tail<BF16>(const IbrlTail&, hipStream_t);

__global__ __launch_bounds__(256) void ibrl_actor_stats_kernel(const IbrlActorStats a) {
  __shared__ double sh[2][256];
  double v[2] = {0.0, 0.0};
  for (int64_t n = threadIdx.x; n < a.N; n += 256) {
    float q = 0.f;
    for (int e = 0; e < a.E; ++e) q += a.q[e * a.q_stride + n * a.ldq];
    v[0] += (double)a.qmin[n], v[1] += (double)(q / (float)a.E);
  }
  sac_tree<2>(sh, v);
  if (threadIdx.x == 0) {
    const double dn = (double)a.N;
    a.stats[0] = -(sh[0][0] / dn), a.stats[1] = sh[0][0] / dn, a.stats[2] = sh[1][0] / dn;
  }
}
void launch_ibrl_actor_stats(const IbrlActorStats& a, hipStream_t s) {
  hipLaunchKernelGGL(ibrl_actor_stats_kernel, dim3(1), dim3(256), 0, s, a);
}

}  // namespace dppo
