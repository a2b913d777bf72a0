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

}  // namespace dppo
