// See dql.h.  gfx950 only.  Compiled with -ffp-contract=off: x_noisy and x0_raw keep torch's op sequence (fp32 products and one
// sum or difference, never an fma); the link's dot product spells its fma out.
#include "dql.h"

namespace dppo {

template <class P>
union DqlChunk {
  typename P::elem_t e[16 / P::ESIZE];
  u32x4 v;
};
static unsigned dql_grid(int64_t items) {
  const int64_t blocks = (items + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks));
}
__device__ __forceinline__ int dql_clamp_t(int64_t t, int K) { return (int)(t < 0 ? 0 : (t >= K ? K - 1 : t)); }

// ---- rows -----------------------------------------------------------------------------------------------------------------
// One thread per 16-byte chunk: first the actor's rows, then the encoder's (if any), then the critic's.
template <class P>
__global__ __launch_bounds__(256) void dql_rows_kernel(const DqlRows a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  const IdqlRows& g = a.ring;
  const int64_t N = g.N, M = (int64_t)(a.K + 1) * N;
  const int OD = g.OD, AF = a.AF;
  const int ca = a.KpA / EPC, cc = a.inC != nullptr ? a.KpC / EPC : 0, cq = a.KpQ / EPC;
  const int64_t nA = M * ca, nC = M * cc, total = nA + nC + N * cq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    DqlChunk<P> ch;
    if (i < nA + nC) {
      const bool isA = i < nA;
      const int64_t q = isA ? i : i - nA;
      const int cpr = isA ? ca : cc;
      const int64_t r = q / cpr;
      const int c0 = (int)(q - r * cpr) * EPC;
      const int s = (int)(r / N);
      const int64_t n = r - (int64_t)s * N;
      const float* ob = g.obs + idql_ring_row(g, n) * OD;
      if (isA) {
        const int t = s < a.K ? a.K - 1 - s : dql_clamp_t(a.t_bc[n], a.K);
        if (c0 == 0) a.krow[r] = t;
        const float* xs = a.chains + (n * (a.K + 1) + s) * AF;  // (s = K: the action a)
#pragma unroll
        for (int k = 0; k < EPC; ++k) {
          const int c = c0 + k;
          float x = 0.f;
          if (c < AF) {
            x = xs[c];
            if (s == a.K) {
              const float p0 = a.sa[t] * x;
              const float p1 = a.sb[t] * a.noise_bc[n * AF + c];
              x = p0 + p1;
            }
          } else if (c < AF + a.td) {
            x = a.temb[(size_t)t * a.td + (c - AF)];
          } else if (c < AF + a.td + OD && a.obs_in_a) {
            x = ob[c - AF - a.td];
          }
          ch.e[k] = P::from_f32(x);
        }
        *(u32x4*)((E*)a.inA + r * a.KpA + c0) = ch.v;
      } else {
#pragma unroll
        for (int k = 0; k < EPC; ++k) ch.e[k] = P::from_f32(c0 + k < OD ? ob[c0 + k] : 0.f);
        *(u32x4*)((E*)a.inC + r * a.KpC + c0) = ch.v;
      }
    } else {
      const int64_t q = i - nA - nC;
      const int64_t n = q / cq;
      const int c0 = (int)(q - n * cq) * EPC;
      const float* ob = g.obs + idql_ring_row(g, n) * OD;
      const float* ac = a.chains + (n * (a.K + 1) + a.K) * AF;
#pragma unroll
      for (int k = 0; k < EPC; ++k) {
        const int c = c0 + k;
        ch.e[k] = P::from_f32(c < OD ? ob[c] : (c < OD + AF ? ac[c - OD] : 0.f));
      }
      *(u32x4*)((E*)a.q1in + n * a.KpQ + c0) = ch.v;
      *(u32x4*)((E*)a.q2in + n * a.KpQ + c0) = ch.v;
    }
  }
}
template <class P>
void launch_dql_rows(const DqlRows& a, hipStream_t s) {
  constexpr int EPC = 16 / P::ESIZE;
  const int64_t M = (int64_t)(a.K + 1) * a.ring.N;
  const int64_t items = M * (a.KpA / EPC) + (a.inC != nullptr ? M * (a.KpC / EPC) : 0) + a.ring.N * (a.KpQ / EPC);
  if (a.ring.N < 1) return;
  hipLaunchKernelGGL((dql_rows_kernel<P>), dim3(dql_grid(items)), dim3(256), 0, s, a);
}
template void launch_dql_rows<F32>(const DqlRows&, hipStream_t);
template void launch_dql_rows<BF16>(const DqlRows&, hipStream_t);

// ---- the posterior's clamp mask ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dql_post_kernel(const DqlPost a) {
  const int64_t total = a.N * a.K * a.AF;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % a.AF);
    const int64_t ns = i / a.AF;
    const int s = (int)(ns % a.K);
    const int64_t n = ns / a.K;
    uint8_t m = 1;
    if (a.has_clip) {
      const dppo_step st = a.tsteps[a.K - 1 - s];
      const float p0 = st.c0 * a.chains[(n * (a.K + 1) + s) * a.AF + j];
      const float p1 = st.c1 * a.eps[((int64_t)s * a.N + n) * a.lde + j];
      m = fabsf(p0 - p1) <= a.clip ? 1 : 0;
    }
    a.mask[i] = m;
  }
}
void launch_dql_post(const DqlPost& a, hipStream_t s) {
  if (a.N < 1) return;
  hipLaunchKernelGGL(dql_post_kernel, dim3(dql_grid(a.N * a.K * a.AF)), dim3(256), 0, s, a);
}

// ---- the BC term ------------------------------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void dql_bc_kernel(const DqlBc a) {
  typedef typename P::elem_t E;
  const float sc = (float)(2.0 / ((double)a.N * a.AF));
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < a.N; n += (int64_t)gridDim.x * 256) {
    double acc = 0.0;
    for (int j = 0; j < a.AF; ++j) {
      const float d = a.eps[n * a.lde + j] - a.noise[n * a.AF + j];
      acc += (double)d * (double)d;
      ((E*)a.d_out)[n * a.ldd + j] = P::from_f32(sc * d);
    }
    a.rowsum[n] = acc;
  }
}
template <class P>
void launch_dql_bc(const DqlBc& a, hipStream_t s) {
  if (a.N < 1) return;
  hipLaunchKernelGGL((dql_bc_kernel<P>), dim3(dql_grid(a.N)), dim3(256), 0, s, a);
}
template void launch_dql_bc<F32>(const DqlBc&, hipStream_t);
template void launch_dql_bc<BF16>(const DqlBc&, hipStream_t);

// ---- statistics and the seed's scale ----------------------------------------------------------------------------------------
// thread i sums rows i, i + 256, ... in double; the 256 partials are added pairwise in a fixed tree: two calls are bit-identical
__global__ __launch_bounds__(256) void dql_stats_kernel(const DqlStats a) {
  __shared__ double sh[5][256];
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t n = threadIdx.x; n < a.N; n += 256) {
    const double q1 = a.q1[n * a.ldq], q2 = a.q2[n * a.ldq];
    v[0] += a.rowsum[n], v[1] += q1, v[2] += q2, v[3] += fabs(q1), v[4] += fabs(q2);
  }
  for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double dn = (double)a.N;
    const double bc = sh[0][0] / (dn * a.AF), m1 = sh[1][0] / dn, m2 = sh[2][0] / dn, a1 = sh[3][0] / dn, a2 = sh[4][0] / dn;
    const double num = a.which == 0 ? m1 : m2, den = a.which == 0 ? a2 : a1;
    const double ql = -num / den;
    a.stats[0] = bc + a.eta * ql, a.stats[1] = bc, a.stats[2] = ql, a.stats[3] = m1, a.stats[4] = m2;
    *a.scale = (float)(-a.eta / (dn * den));
  }
}
void launch_dql_stats(const DqlStats& a, hipStream_t s) { hipLaunchKernelGGL(dql_stats_kernel, dim3(1), dim3(256), 0, s, a); }

// ---- the x / action columns of a first layer -----------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void dql_pack_cols_kernel(const float* w0, int in_dim, int col0, int ncols, int H,
                                                             typename P::elem_t* wa) {
  const int total = ncols * H;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int j = i / H, h = i - j * H;
    wa[i] = P::from_f32(w0[(int64_t)h * in_dim + col0 + j]);
  }
}
template <class P>
void launch_dql_pack_cols(const float* w0, int in_dim, int col0, int ncols, int H, void* wa, hipStream_t s) {
  hipLaunchKernelGGL((dql_pack_cols_kernel<P>), dim3(dql_grid((int64_t)ncols * H)), dim3(256), 0, s, w0, in_dim, col0, ncols, H,
                     (typename P::elem_t*)wa);
}
template void launch_dql_pack_cols<F32>(const float*, int, int, int, int, void*, hipStream_t);
template void launch_dql_pack_cols<BF16>(const float*, int, int, int, int, void*, hipStream_t);

// ---- the link ---------------------------------------------------------------------------------------------------------------
// `rows` rows of dh per block as fp32 in LDS (row stride H + 4 floats, as qsm_tail_kernel); thread o of the block's rows * AF
// outputs walks K = H in index order with one fma per element: a row's result depends on that row alone.
template <class P>
__global__ __launch_bounds__(256) void dql_link_kernel(const DqlLink a) {
  typedef typename P::elem_t E;
  constexpr int EPC = 16 / P::ESIZE;
  extern __shared__ float dql_xs[];
  const int H = a.H, LD = H + 4, AF = a.AF, cpr = H / EPC;
  const int64_t row0 = (int64_t)blockIdx.x * a.rows;
  for (int i = threadIdx.x; i < a.rows * cpr; i += 256) {
    const int r = i / cpr, c = i - r * cpr;
    DqlChunk<P> ch;
    if (row0 + r < a.N)
      ch.v = *(const u32x4*)((const E*)a.dh + (row0 + r) * a.ldh + c * EPC);
    else
      ch.v = u32x4{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < EPC; ++k) dql_xs[r * LD + c * EPC + k] = P::to_f32(ch.e[k]);
  }
  __syncthreads();
  for (int o = threadIdx.x; o < a.rows * AF; o += 256) {
    const int r = o / AF, j = o - r * AF;
    const int64_t n = row0 + r;
    if (n >= a.N) break;
    const float* x = dql_xs + r * LD;
    const E* w = (const E*)a.wa + (int64_t)j * H;
    float acc = 0.f;
    for (int k = 0; k < H; k += EPC) {
      DqlChunk<P> wc;
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
    const int64_t o_dx = n * AF + j;
    float v;
    if (a.mode == 0) {
      v = *a.scale * acc;
    } else if (a.mode == 1) {
      const float t1 = a.sa[dql_clamp_t(a.t_bc[n], a.K)] * acc;
      v = a.dx[o_dx] + t1;
      if (a.d_a != nullptr) a.d_a[o_dx] = v;
      if (a.final_clip && !(fabsf(a.a[n * (a.K + 1) * AF + j]) < 1.f)) v = 0.f;
    } else {
      const dppo_step cur = a.tsteps[a.K - 1 - a.p];
      const float f = a.mask[(n * a.K + a.p) * AF + j] ? cur.c3 + cur.c2 * cur.c0 : cur.c3;
      const float t1 = f * a.dx[o_dx];
      v = t1 + acc;
    }
    a.dx[o_dx] = v;
    if (a.d_out_prev != nullptr) {
      const dppo_step prev = a.tsteps[a.K - a.p];
      const float de = a.mask[(n * a.K + a.p - 1) * AF + j] ? -(prev.c1 * prev.c2) * v : 0.f;
      ((E*)a.d_out_prev)[n * a.ldd + j] = P::from_f32(de);
    }
  }
}
template <class P>
void launch_dql_link(const DqlLink& a, hipStream_t s) {
  if (a.N < 1 || a.rows < 1) return;
  const unsigned blocks = (unsigned)((a.N + a.rows - 1) / a.rows);
  hipLaunchKernelGGL((dql_link_kernel<P>), dim3(blocks), dim3(256), (size_t)a.rows * (a.H + 4) * 4, s, a);
}
template void launch_dql_link<F32>(const DqlLink&, hipStream_t);
template void launch_dql_link<BF16>(const DqlLink&, hipStream_t);

}  // namespace dppo
