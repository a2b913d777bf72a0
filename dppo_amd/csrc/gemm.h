// MFMA GEMM kernels for the big-batch side of the DPPO path (log-prob precompute, PPO update).
//
//  gemm_nt : Y[M,N] = epi( X[M,Kp] . W[N,Kp]^T )          forward layers and backward-data
//  gemm_tn : C[N1,N2] (+)= A[M,N1]^T . B[M,N2]             weight gradients, split over M into slabs
//
// Both are written "transposed": the MFMA's 16-row operand (A) is the weight / gradient-feature
// side and its 16-column operand (B) is the batch-row side, so every lane ends up owning ONE batch
// row and a run of 4*TN consecutive features -- epilogue loads/stores are 16-byte vectors and one
// wave instruction covers 16 rows x 128 contiguous bytes.
#pragma once
#include "common.h"

namespace dppo {

struct GemmNT {
  const void* X;  // [M][ldx] elem (row-major), columns >= Kp never read
  const void* W;  // [N][ldw] elem (nn.Linear layout), rows >= N treated as zero
  const float* bias;  // [N] or null
  int M, N, Kp;       // Kp: multiple of 128 bytes / esize
  int ldx, ldw;
  // epilogue, in this order:  v = acc + bias;  v *= act'(dsrc);  v += res + add;  stores
  const void* dsrc;  // pre-activation the derivative is taken at: f32 (dsrc_kind 1) or elem (2)
  int dsrc_kind, dsrc_ld, dact;
  const float* res;  // f32 addend [M][ldres]
  int ldres;
  const void* add;  // elem addend [M][ldadd]
  int ldadd;
  float* out_f32;  // [M][ldo32]
  int ldo32;
  void* out_pre;  // elem(v)        [M][ldo]
  void* out_act;  // elem(act(v))   [M][ldo]
  int ldo, act;
};

struct GemmTN {
  const void* A;  // [M][lda] elem ; contributes rows of C (N1)
  const void* B;  // [M][ldb] elem ; contributes columns of C (N2)
  int M, N1, N2, lda, ldb;
  float* slab;  // [splits][N1][ldc] partial sums
  int ldc, splits, rows_per_split;  // rows_per_split multiple of 64
  // readable columns of a row when they differ from its stride (0 = lda / ldb): rows may OVERLAP -- an im2col operand
  // that is a window of stride C and width k*C over a channel-last image (unet.hip).  Register-staged kernel only.
  int ncol_a, ncol_b;
};

constexpr int MAX_TN_JOBS = 8;
struct GemmTNGroup {  // one launch over the 128 x 128 tiles of n weight-gradient GEMMs (gemm_tn_group_kernel)
  GemmTN j[MAX_TN_JOBS];
  int base[MAX_TN_JOBS + 1];  // first workgroup of job i; base[n] = grid size
  int n;
};

template <class P>
void launch_gemm_nt(const GemmNT& a, hipStream_t s);
template <class P>
void launch_gemm_tn_group(const GemmTNGroup& gr, hipStream_t s);
// Orders the n jobs of a group for launch_gemm_tn_group (longest row ranges first: the short jobs fill the last round) and
// fills base[]
void gemm_tn_group_order(GemmTNGroup& gr);
void set_gemm_tn_variant(int v);  // tuning knob 5
void set_gemm_tn_nbuf(int v);     // tuning knob 26
void set_gemm_tn_thin(int v);     // tuning knob 6

// Measurement hook (bench.py's roofline): while armed for a kernel id, every launch of that kernel is bracketed by
// HIP events recorded on its launch stream.  Process-wide, not thread-safe, off by default; never armed by the
// product path.
enum { PROBE_GEMM_NT_HIDDEN = 1, PROBE_GEMM_TN = 2, PROBE_FUSED_FWD = 3, PROBE_FUSED_BWD = 4, PROBE_SAMPLER = 5 };
void set_gemm_nt_variant(int v);  // 0 register staging, 1 LDS-DMA staging where legal (default)
void set_gemm_nt_small(int v);    // 1 (default): 64 x 64 / 64 x 32 tiles when 128 x 128 tiles would give < 192 workgroups
int probe_arm(int kernel_id, int max_launches);
int probe_collect(double* total_ms, int* launches, double* flops, double* bytes = nullptr);
bool probe_begin(int kernel_id, hipStream_t s);  // true if this launch is being timed
void probe_end(hipStream_t s, double flops, double bytes = 0);  // right after the launch when probe_begin returned true
template <class P>
void launch_gemm_tn(const GemmTN& a, hipStream_t s);
bool gemm_tn_thin(int N1, int N2);  // true: the 512 x 64 block shape is used (one output tile covers <= 64 columns)

// out[n] (+)= sum_s slab[s][n]  (fixed order => reproducible)
void launch_slab_reduce(const float* slab, int splits, size_t n, float* out, float scale, hipStream_t s);
// colsum[j] = sum_m A[m][j] for j < N ; deterministic two-stage
template <class P>
void launch_colsum(const void* A, int M, int N, int lda, float* partial /*[blocks][N]*/, int blocks, float* out,
                   float scale, hipStream_t s);

}  // namespace dppo
