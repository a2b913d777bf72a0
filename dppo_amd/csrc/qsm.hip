// See qsm.h.  gfx950 only.  Compiled with -ffp-contract=off: q_sample keeps torch's op sequence (two fp32 products and one sum,
// never an fma); the tail's dot product spells its fma out.
#include "qsm.h"

namespace dppo {

template <class P>
union QsmChunk {
  typename P::elem_t e[16 / P::ESIZE];
  u32x4 v;
};

// ---- row builders ---------------------------------------------------------------------------------------------------------
// One thread per 16-byte chunk of a row's operand image; the thread that owns a column also writes its fp32 copies (obs_out,
// pairs[:, 0]): every column of [obs | x_t] is below in_dim <= KpQ, so each is written exactly once.
template <class P>
__global__ __launch_bounds__(256) void qsm_rows_kernel(const QsmRows a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const IdqlRows& g = a.ring;
  const int W = a.KpQ / EPC, OD = g.OD, AD = g.AD;
  const int64_t total = g.N * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / W;
    const int c = (int)(i - n * W);
    const int64_t row = idql_ring_row(g, n);
    int64_t tt = a.t[n];
    tt = tt < 0 ? 0 : (tt >= a.K ? a.K - 1 : tt);
    const float sa = a.sa[tt], sb = a.sb[tt];
    QsmChunk<P> ch;
#pragma unroll
    for (int k = 0; k < EPC; ++k) {
      const int col = c * EPC + k;
      float x = 0.f;
      if (col < OD) {
        x = g.obs[row * OD + col];
        a.obs_out[n * OD + col] = x;
      } else if (col < OD + AD) {
        const int j = col - OD;
        const float p0 = sa * g.actions[row * AD + j];
        const float p1 = sb * a.noise[n * AD + j];
        x = p0 + p1;
        a.pairs[n * 2 * AD + j] = x;
      }
      ch.e[k] = P::from_f32(x);
    }
    *(u32x4*)((E*)a.q1in + n * a.KpQ + c * EPC) = ch.v;
    *(u32x4*)((E*)a.q2in + n * a.KpQ + c * EPC) = ch.v;
  }
}
static unsigned qsm_grid(int64_t items) {
  const int64_t blocks = (items + 255) / 256;
  return (unsigned)(blocks > 2048 ? 2048 : blocks);
}
template <class P>
void launch_qsm_rows(const QsmRows& a, hipStream_t s) {
  const int64_t items = a.ring.N * (a.KpQ / (16 / P::ESIZE));
  if (items < 1) return;
  hipLaunchKernelGGL((qsm_rows_kernel<P>), dim3(qsm_grid(items)), dim3(256), 0, s, a);
}
template void launch_qsm_rows<F32>(const QsmRows&, hipStream_t);
template void launch_qsm_rows<BF16>(const QsmRows&, hipStream_t);

template <class P>
__global__ __launch_bounds__(256) void qsm_td_rows_kernel(const QsmTdRows a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const IdqlRows& g = a.ring;
  const int W = a.KpQ / EPC, OD = g.OD, AD = g.AD;
  const int64_t total = g.N * 2 * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / (2 * W);
    int c = (int)(i - n * 2 * W);
    const bool nxt = c >= W;
    if (nxt) c -= W;
    const int64_t row = idql_ring_row(g, n);
    if (c == 0 && !nxt) {
      a.r_out[n] = g.reward[row];
      a.term_out[n] = g.terminated[row];
    }
    const float* ob = (nxt ? g.next_obs : g.obs) + row * OD;
    const float* ac = nxt ? a.next_actions + n * AD : g.actions + row * AD;
    QsmChunk<P> ch;
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
    *(u32x4*)((E*)(nxt ? a.t1in : a.q1in) + n * a.KpQ + c * EPC) = ch.v;
    *(u32x4*)((E*)(nxt ? a.t2in : a.q2in) + n * a.KpQ + c * EPC) = ch.v;
  }
}
template <class P>
void launch_qsm_td_rows(const QsmTdRows& a, hipStream_t s) {
  const int64_t items = a.ring.N * 2 * (a.KpQ / (16 / P::ESIZE));
  if (items < 1) return;
  hipLaunchKernelGGL((qsm_td_rows_kernel<P>), dim3(qsm_grid(items)), dim3(256), 0, s, a);
}
template void launch_qsm_td_rows<F32>(const QsmTdRows&, hipStream_t);
template void launch_qsm_td_rows<BF16>(const QsmTdRows&, hipStream_t);

// ---- the data-gradient chain's seed ---------------------------------------------------------------------------------------
// d q / d z1_last = Wout (.) act'(z1_last): what gemm_nt's epilogue would make of d_out = 1 times Wout^T, without the GEMM
template <class P>
__global__ __launch_bounds__(256) void qsm_seed_kernel(const void* wout, const void* z, int64_t N, int H, int act, void* dz) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const int W = H / EPC;
  const int64_t total = N * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % W);
    QsmChunk<P> w, x, o;
    w.v = *(const u32x4*)((const E*)wout + c * EPC);
    x.v = *(const u32x4*)((const E*)z + i * EPC);
#pragma unroll
    for (int k = 0; k < EPC; ++k) o.e[k] = P::from_f32(P::to_f32(w.e[k]) * act_grad_f(act, P::to_f32(x.e[k])));
    *(u32x4*)((E*)dz + i * EPC) = o.v;
  }
}
template <class P>
void launch_qsm_seed(const void* wout, const void* z, int64_t N, int H, int act, void* dz, hipStream_t s) {
  const int64_t items = N * (H / (16 / P::ESIZE));
  if (items < 1) return;
  hipLaunchKernelGGL((qsm_seed_kernel<P>), dim3(qsm_grid(items)), dim3(256), 0, s, wout, z, N, H, act, dz);
}
template void launch_qsm_seed<F32>(const void*, const void*, int64_t, int, int, void*, hipStream_t);
template void launch_qsm_seed<BF16>(const void*, const void*, int64_t, int, int, void*, hipStream_t);

// ---- the tail ---------------------------------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void pack_w0a_kernel(const float* params, int64_t stride, int64_t w0_off, int in_dim, int OD, int AF,
                                                        int H, int E, typename P::elem_t* wa) {
  const int K = E * H, total = AF * K;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int a = i / K, k = i - a * K;
    const int e = k / H, h = k - e * H;
    wa[i] = P::from_f32(params[e * stride + w0_off + (int64_t)h * in_dim + OD + a]);
  }
}
template <class P>
void launch_pack_w0a(const float* params, int64_t stride, int64_t w0_off, int in_dim, int OD, int AF, int H, int E, void* wa,
                     hipStream_t s) {
  const int blocks = (AF * E * H + 255) / 256;
  hipLaunchKernelGGL((pack_w0a_kernel<P>), dim3(blocks > 2048 ? 2048 : blocks), dim3(256), 0, s, params, stride, w0_off, in_dim, OD, AF,
                     H, E, (typename P::elem_t*)wa);
}
template void launch_pack_w0a<F32>(const float*, int64_t, int64_t, int, int, int, int, int, void*, hipStream_t);
template void launch_pack_w0a<BF16>(const float*, int64_t, int64_t, int, int, int, int, int, void*, hipStream_t);

// `rows` rows of dh per block as fp32 in LDS (row stride H2 + 4 floats: rows that differ by one land four banks apart, so
// the 16-byte reads of a wave that spans several rows do not collide); thread o of the block's rows * AD outputs walks K = 2H in
// index order with one fma per element: a row's result does not depend on which block or which call it is in.
constexpr int QSM_TAIL_LDS = 48 * 1024;
int qsm_tail_rows(int H2) {
  const int r = QSM_TAIL_LDS / ((H2 + 4) * 4);
  return r > 16 ? 16 : r;
}
template <class P>
__global__ __launch_bounds__(256) void qsm_tail_kernel(const QsmTail a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  extern __shared__ float qsm_xs[];
  const int H2 = a.H2, LD = H2 + 4, AD = a.AD, cpr = H2 / EPC;
  const int64_t row0 = (int64_t)blockIdx.x * a.rows;
  for (int i = threadIdx.x; i < a.rows * cpr; i += 256) {
    const int r = i / cpr, c = i - r * cpr;
    QsmChunk<P> ch;
    if (row0 + r < a.N)
      ch.v = *(const u32x4*)((const E*)a.dh + (row0 + r) * H2 + c * EPC);
    else
      ch.v = u32x4{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < EPC; ++k) qsm_xs[r * LD + c * EPC + k] = P::to_f32(ch.e[k]);
  }
  __syncthreads();
  const float scale = -a.coeff;
  for (int o = threadIdx.x; o < a.rows * AD; o += 256) {
    const int r = o / AD, j = o - r * AD;
    const int64_t n = row0 + r;
    if (n >= a.N) break;
    const float* x = qsm_xs + r * LD;
    const E* w = (const E*)a.wa + (int64_t)j * H2;
    float acc = 0.f;
    for (int k = 0; k < H2; k += EPC) {
      QsmChunk<P> wc;
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
    const float gm = acc * 0.5f;  // mean of the two trunks' gradients: the K = 2H sum is g_1 + g_2
    a.pairs[(n * 2 + 1) * AD + j] = scale * gm;
    if (a.g_out != nullptr) a.g_out[n * AD + j] = gm;
  }
}
template <class P>
void launch_qsm_tail(const QsmTail& a, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.N + a.rows - 1) / a.rows);
  hipLaunchKernelGGL((qsm_tail_kernel<P>), dim3(blocks), dim3(256), (size_t)a.rows * (a.H2 + 4) * 4, s, a);
}
template void launch_qsm_tail<F32>(const QsmTail&, hipStream_t);
template void launch_qsm_tail<BF16>(const QsmTail&, hipStream_t);

}  // namespace dppo
