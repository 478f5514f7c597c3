// CDNA4 (gfx950) kernels for synchronized batch normalisation, forward and
// backward, around the two SUM-allreduces of contrib/sync_batchnorm.py.
//
// The torch chain makes some thirty passes over the activation with f32
// temporaries of its size. The algorithm needs three passes forward (read x,
// read x, write y) and five backward (read dy and x twice, write dx), in the
// input's own dtype. Four kernel roles, each followed or preceded by the
// allreduce of a C-sized f32 vector:
//
//   bn_stats        partial sum(x), sum(x*x) per channel        } stats[2C+1]
//   bn_finalize     fixed-order sum of the partials, + count    }
//   bn_apply        mean, var, invstd from the reduced stats in registers;
//                   y = (x - mean) * invstd * w + b; one block per channel
//                   (tile) also stores mean/invstd for backward and updates
//                   the running statistics
//   bn_bwd_reduce   partial sum(dy), sum(dy * (x - mean))       } packed[2C],
//   bn_finalize     the same second stage; also grad_weight,    } gw, gb
//                   grad_bias from the local sums
//   bn_bwd_apply    dx = (dy - S1/n - (x - mean) * invstd^2 * S2/n)
//                        * invstd * w
//
// An activation can be fused into three of the roles (template parameter
// ACT: none, ReLU, or add a residual z and ReLU):
//
//   bn_apply        y = relu((x - mean) * invstd * w + b [+ z]), the add in
//                   f32 before the one rounding; NaN passes as in torch.relu
//   bn_bwd_reduce   the sums of d = (y > 0) ? dy : 0 in place of dy
//   bn_bwd_apply    dx from d, and dz = d where the residual wants it
//
// Backward needs only the sign of the stored y. In the rows layout the
// forward writes it as one byte per 16-byte vector, [rows, C / V] (bit k
// is element k of the vector, so f32 uses four bits), from the thread that
// holds the vector: neighbouring channel lanes write neighbouring bytes,
// and backward reads a sixteenth of y's bytes. In the planes layout, whose
// element loads have no natural byte, backward reads y itself.
//
// All arithmetic is f32; outputs are rounded once (bf16 as torch rounds).
// Sums are deterministic, no float atomics: per-thread partial sums, a
// fixed-order reduction inside the block into its row of a [blocks, 2C] f32
// buffer, and bn_finalize, which adds the rows in a fixed order. Beyond a
// thread's own run of elements every level adds pairwise, so the error
// grows with the logarithm of the count, as that of torch's sums does.
//
// Two layouts of the same [N, C, S] problem:
//
//  rows    [rows, C]: channels-last 4-d input (rows = N*H*W) and S == 1.
//          As in epilogue_kernels.hip a 256-thread block is CVT lanes along
//          C (V elements = 16 bytes per lane) times RL = 256 / CVT
//          row-lanes, and a thread keeps its channels for the whole kernel:
//          per-channel scalars and partial sums live in registers. Grids
//          are capped and grid-stride over rows. More than 256 channel
//          vectors are tiled over gridDim.y. Needs C % V == 0 and 16-byte
//          aligned bases.
//  planes  [N, C, S], S > 1, NCHW-contiguous. Block column c (blockIdx.x)
//          works on channel c; its gridDim.y blocks split the channel's
//          N * S / V load units. V is 16 bytes' worth when S * sizeof(T) is
//          a multiple of 16 and the bases are aligned, else 1: any C and S.
//          Block sums are wave64 shuffles, then LDS across the four waves.

#include <hip/hip_runtime.h>  // by name in every .hip file: see device_util.h
#include <cmath>

#include "device_util.h"  // to_f / from_f (bf16 is bf16_t), NO_PACKED_F32
#include "launchers.h"

#define BN_BLOCK 256
// row-blocks of the rows-layout apply kernels
#define BN_APPLY_MAX_GRID 2048
// finalize: 8 channels x 32 slices of the partial rows per block
#define BN_FIN_CH 8
#define BN_FIN_SL (BN_BLOCK / BN_FIN_CH)
// planes: a channel gets one block per this many loads of each thread, up
// to BN_PLANE_MAX_BLOCKS blocks over all channels and BN_PLANE_MAX_SPLITS
// per channel
#define BN_PLANE_LOADS 4
#define BN_PLANE_MAX_BLOCKS 2048
#define BN_PLANE_MAX_SPLITS 512

// Like the newer kernels of kernels.hip, these are built without packed
// f32 arithmetic; they are bound by memory and lose nothing by it.
#define BN_KERNEL \
  __global__ void __launch_bounds__(BN_BLOCK) NO_PACKED_F32

namespace {

// V elements loaded at once: 16 bytes, or one element
template <typename T, int V> struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

// A per-channel vector (weight, bias, running statistics, their gradients)
// is f32 or T, told at run time: under autocast the activation is bf16 and
// the parameters stay f32. Element access: such a tensor may be a view into
// a flat parameter buffer and need not be aligned.
template <typename T>
__device__ __forceinline__ float ld_param(const void* p, int is_f32, int i) {
  return is_f32 ? static_cast<const float*>(p)[i]
                : to_f(static_cast<const T*>(p)[i]);
}
template <typename T>
__device__ __forceinline__ void st_param(void* p, int is_f32, int i,
                                         float v) {
  if (is_f32)
    static_cast<float*>(p)[i] = v;
  else
    static_cast<T*>(p)[i] = from_f<T>(v);
}

// what bn_apply takes besides the data
struct ApplyParams {
  const void* w;  // each of w, b, rmean/rvar may be null
  const void* b;
  void* rmean;
  void* rvar;
  int w_f32, b_f32, r_f32;
  float momentum, one_minus_momentum, eps;
};

struct Moments {
  float mean, var, invstd, count;
};

// from the allreduced stats = (sum[C], sqsum[C], count)
__device__ __forceinline__ Moments moments_of(const float* __restrict__ stats,
                                              int C, int c, float eps) {
  Moments m;
  m.count = stats[2 * C];
  m.mean = stats[c] / m.count;
  m.var = fmaxf(stats[C + c] / m.count - m.mean * m.mean, 0.f);
  m.invstd = 1.f / sqrtf(m.var + eps);
  return m;
}

// One thread per channel does this in bn_apply: keep mean and invstd for
// backward, move the running statistics (unbiased variance).
template <typename T>
__device__ __forceinline__ void keep_moments(const Moments& m, int C, int c,
                                             float* __restrict__ mean_invstd,
                                             const ApplyParams& p) {
  mean_invstd[c] = m.mean;
  mean_invstd[C + c] = m.invstd;
  if (p.rmean) {
    const float unbiased = m.var * m.count / (m.count - 1.f);
    st_param<T>(p.rmean, p.r_f32, c,
                p.one_minus_momentum * ld_param<T>(p.rmean, p.r_f32, c) +
                    p.momentum * m.mean);
    st_param<T>(p.rvar, p.r_f32, c,
                p.one_minus_momentum * ld_param<T>(p.rvar, p.r_f32, c) +
                    p.momentum * unbiased);
  }
}

// the activation fused into bn_apply; the backward kernels only know
// whether there was one (MASKED)
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_ADD_RELU = 2 };

// max(v, 0) that lets NaN through as torch.relu does; fmaxf would drop it
__device__ __forceinline__ float relu_keep_nan(float v) {
  return (v > 0.f || v != v) ? v : 0.f;
}

// ---------------------------------------------------------------------------
// rows layout
// ---------------------------------------------------------------------------

struct RowsGeom {
  int C;      // channels
  int CVtot;  // channel vectors of a row, C / V
  int CVT;    // lanes along C of a block (channel vectors of a tile)
  int RL;     // row-lanes of a block, BN_BLOCK / CVT
};

// A thread's place: channel vector cv of the row, row-lane tr.
struct RowLane {
  int tc, tr, cv;
  bool active;
};

__device__ __forceinline__ RowLane row_lane(const RowsGeom& g) {
  RowLane l;
  l.tc = threadIdx.x % g.CVT;
  l.tr = threadIdx.x / g.CVT;
  l.cv = blockIdx.y * g.CVT + l.tc;
  l.active = l.tr < g.RL && l.cv < g.CVtot;
  return l;
}

// Sum the row-lanes' two partials pairwise (a fixed tree: lane t takes lane
// t + ceil(n / 2) until one is left, which keeps the error of a long sum
// down) and store them into the block's row [2C] of the partial buffer.
// Every thread of the block calls.
template <int V>
__device__ __forceinline__ void rows_block_reduce_store(
    const float (&a)[V], const float (&b)[V], const RowLane& l,
    const RowsGeom& g, float* __restrict__ partial_row) {
  __shared__ float red[2][BN_BLOCK * V];
  const int Ct = g.CVT * V;  // channels of a tile; RL * Ct <= BN_BLOCK * V
  if (l.active) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      red[0][l.tr * Ct + l.tc * V + k] = a[k];
      red[1][l.tr * Ct + l.tc * V + k] = b[k];
    }
  }
  __syncthreads();
  // columns past C of a narrower last tile hold nothing and go nowhere
  for (int n = g.RL; n > 1;) {
    const int h = (n + 1) / 2;
    for (int i = threadIdx.x; i < (n - h) * Ct; i += BN_BLOCK) {
      red[0][i] += red[0][i + h * Ct];
      red[1][i] += red[1][i + h * Ct];
    }
    __syncthreads();
    n = h;
  }
  for (int j = threadIdx.x; j < Ct; j += BN_BLOCK) {
    const int c = blockIdx.y * Ct + j;
    if (c >= g.C) break;
    partial_row[c] = red[0][j];
    partial_row[g.C + c] = red[1][j];
  }
}

template <typename T>
BN_KERNEL bn_rows_stats_kernel(const T* __restrict__ x,
                               float* __restrict__ partial, size_t rows,
                               RowsGeom g) {
  using VT = Pack<T, 16 / sizeof(T)>;
  constexpr int V = 16 / sizeof(T);
  const RowLane l = row_lane(g);
  float s[V], q[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s[k] = q[k] = 0.f;
  if (l.active) {
    const VT* xv = reinterpret_cast<const VT*>(x) + l.cv;
    const size_t stride = (size_t)gridDim.x * g.RL;
#pragma unroll 4
    for (size_t r = (size_t)blockIdx.x * g.RL + l.tr; r < rows; r += stride) {
      const VT a = xv[r * g.CVtot];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float f = to_f(a.v[k]);
        s[k] += f;
        q[k] += f * f;
      }
    }
  }
  rows_block_reduce_store<V>(s, q, l, g,
                             partial + (size_t)blockIdx.x * 2 * g.C);
}

// ACT != none: z is the residual (add+ReLU only) and mask gets a byte per
// vector of the stored y, bit k set where element k is above zero.
template <typename T, int ACT>
BN_KERNEL bn_rows_apply_kernel(const T* __restrict__ x,
                               const T* __restrict__ z, T* __restrict__ y,
                               uint8_t* __restrict__ mask,
                               const float* __restrict__ stats,
                               float* __restrict__ mean_invstd, size_t rows,
                               RowsGeom g, ApplyParams p) {
  using VT = Pack<T, 16 / sizeof(T)>;
  constexpr int V = 16 / sizeof(T);
  const RowLane l = row_lane(g);
  if (!l.active) return;
  float mean[V], invstd[V], w[V], b[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int c = l.cv * V + k;
    const Moments m = moments_of(stats, g.C, c, p.eps);
    mean[k] = m.mean;
    invstd[k] = m.invstd;
    w[k] = p.w ? ld_param<T>(p.w, p.w_f32, c) : 1.f;
    b[k] = p.b ? ld_param<T>(p.b, p.b_f32, c) : 0.f;
    if (blockIdx.x == 0 && l.tr == 0)
      keep_moments<T>(m, g.C, c, mean_invstd, p);
  }
  const VT* xv = reinterpret_cast<const VT*>(x) + l.cv;
  const VT* zv = reinterpret_cast<const VT*>(z);
  VT* yv = reinterpret_cast<VT*>(y) + l.cv;
  const size_t stride = (size_t)gridDim.x * g.RL;
#pragma unroll 4
  for (size_t r = (size_t)blockIdx.x * g.RL + l.tr; r < rows; r += stride) {
    VT a = xv[r * g.CVtot];
    if constexpr (ACT == ACT_NONE) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        a.v[k] =
            from_f<T>((to_f(a.v[k]) - mean[k]) * invstd[k] * w[k] + b[k]);
    } else {
      VT res;
      if constexpr (ACT == ACT_ADD_RELU) res = zv[r * g.CVtot + l.cv];
      unsigned bits = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float v = (to_f(a.v[k]) - mean[k]) * invstd[k] * w[k] + b[k];
        if constexpr (ACT == ACT_ADD_RELU) v += to_f(res.v[k]);
        a.v[k] = from_f<T>(relu_keep_nan(v));
        // the sign of what is stored: a small v may round to zero
        bits |= (unsigned)(to_f(a.v[k]) > 0.f) << k;
      }
      mask[r * g.CVtot + l.cv] = (uint8_t)bits;
    }
    yv[r * g.CVtot] = a;
  }
}

// MASKED: dy counts only where its bit of the forward's mask is set
template <typename T, bool MASKED>
BN_KERNEL bn_rows_bwd_reduce_kernel(const T* __restrict__ dy,
                                    const T* __restrict__ x,
                                    const uint8_t* __restrict__ mask,
                                    const float* __restrict__ mean_invstd,
                                    float* __restrict__ partial, size_t rows,
                                    RowsGeom g) {
  using VT = Pack<T, 16 / sizeof(T)>;
  constexpr int V = 16 / sizeof(T);
  const RowLane l = row_lane(g);
  float s1[V], s2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s1[k] = s2[k] = 0.f;
  if (l.active) {
    float mean[V];
#pragma unroll
    for (int k = 0; k < V; ++k) mean[k] = mean_invstd[l.cv * V + k];
    const VT* gv = reinterpret_cast<const VT*>(dy) + l.cv;
    const VT* xv = reinterpret_cast<const VT*>(x) + l.cv;
    const size_t stride = (size_t)gridDim.x * g.RL;
#pragma unroll 2
    for (size_t r = (size_t)blockIdx.x * g.RL + l.tr; r < rows; r += stride) {
      const VT d = gv[r * g.CVtot];
      const VT a = xv[r * g.CVtot];
      unsigned bits = 0;
      if constexpr (MASKED) bits = mask[r * g.CVtot + l.cv];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float f = to_f(d.v[k]);
        if constexpr (MASKED) f = (bits >> k & 1u) ? f : 0.f;
        s1[k] += f;
        s2[k] += f * (to_f(a.v[k]) - mean[k]);
      }
    }
  }
  rows_block_reduce_store<V>(s1, s2, l, g,
                             partial + (size_t)blockIdx.x * 2 * g.C);
}

// per-channel coefficients of dx = (dy - k1 - (x - mean) * k2) * scale
struct BwdCoef {
  float mean, k1, k2, scale;
};

template <typename T>
__device__ __forceinline__ BwdCoef bwd_coef(
    const float* __restrict__ packed, const float* __restrict__ stats,
    const float* __restrict__ mean_invstd, const void* w, int w_f32, int C,
    int c) {
  const float count = stats[2 * C];
  const float invstd = mean_invstd[C + c];
  BwdCoef k;
  k.mean = mean_invstd[c];
  k.k1 = packed[c] / count;
  k.k2 = invstd * invstd * packed[C + c] / count;
  k.scale = w ? invstd * ld_param<T>(w, w_f32, c) : invstd;
  return k;
}

// MASKED: as above; the masked dy is also the residual's gradient and is
// stored to dz where that is not null
template <typename T, bool MASKED>
BN_KERNEL bn_rows_bwd_apply_kernel(const T* __restrict__ dy,
                                   const T* __restrict__ x,
                                   const uint8_t* __restrict__ mask,
                                   T* __restrict__ dx, T* __restrict__ dz,
                                   const float* __restrict__ packed,
                                   const float* __restrict__ stats,
                                   const float* __restrict__ mean_invstd,
                                   const void* __restrict__ w, int w_f32,
                                   size_t rows, RowsGeom g) {
  using VT = Pack<T, 16 / sizeof(T)>;
  constexpr int V = 16 / sizeof(T);
  const RowLane l = row_lane(g);
  if (!l.active) return;
  float mean[V], k1[V], k2[V], scale[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const BwdCoef co = bwd_coef<T>(packed, stats, mean_invstd, w, w_f32, g.C,
                                   l.cv * V + k);
    mean[k] = co.mean;
    k1[k] = co.k1;
    k2[k] = co.k2;
    scale[k] = co.scale;
  }
  const VT* gv = reinterpret_cast<const VT*>(dy) + l.cv;
  const VT* xv = reinterpret_cast<const VT*>(x) + l.cv;
  VT* dv = reinterpret_cast<VT*>(dx) + l.cv;
  VT* zv = reinterpret_cast<VT*>(dz);
  const size_t stride = (size_t)gridDim.x * g.RL;
#pragma unroll 2
  for (size_t r = (size_t)blockIdx.x * g.RL + l.tr; r < rows; r += stride) {
    VT d = gv[r * g.CVtot];
    const VT a = xv[r * g.CVtot];
    if constexpr (MASKED) {
      const unsigned bits = mask[r * g.CVtot + l.cv];
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (!(bits >> k & 1u)) d.v[k] = from_f<T>(0.f);
      if (dz) zv[r * g.CVtot + l.cv] = d;
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
      d.v[k] = from_f<T>(
          (to_f(d.v[k]) - k1[k] - (to_f(a.v[k]) - mean[k]) * k2[k]) *
          scale[k]);
    dv[r * g.CVtot] = d;
  }
}

// ---------------------------------------------------------------------------
// planes layout
// ---------------------------------------------------------------------------

struct PlaneGeom {
  uint32_t C;
  uint32_t SV;  // load units of one plane, S / V
  uint32_t M;   // load units of one channel, N * SV
};

// where unit i of channel c starts, in units
__device__ __forceinline__ size_t plane_unit(uint32_t i, uint32_t c,
                                             const PlaneGeom& g) {
  const uint32_t n = i / g.SV;
  const uint32_t j = i - n * g.SV;
  return ((size_t)n * g.C + c) * g.SV + j;
}

// The block's sums of a[] and b[], in a[0] and b[0] of thread 0, all
// pairwise: the thread's V accumulators, wave64 shuffles, then the four
// waves' results through LDS. Every thread of the block calls.
template <int V>
__device__ __forceinline__ void plane_block_sum(float (&av)[V],
                                                float (&bv)[V]) {
  __shared__ float red[2][BN_BLOCK / 64];
#pragma unroll
  for (int h = V / 2; h > 0; h /= 2) {
#pragma unroll
    for (int k = 0; k < h; ++k) {
      av[k] += av[k + h];
      bv[k] += bv[k + h];
    }
  }
  float a = av[0], b = bv[0];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    av[0] = (red[0][0] + red[0][2]) + (red[0][1] + red[0][3]);
    bv[0] = (red[1][0] + red[1][2]) + (red[1][1] + red[1][3]);
  }
}

template <typename T, int V>
BN_KERNEL bn_planes_stats_kernel(const T* __restrict__ x,
                                 float* __restrict__ partial, PlaneGeom g) {
  using VT = Pack<T, V>;
  const uint32_t c = blockIdx.x;
  const VT* xv = reinterpret_cast<const VT*>(x);
  float s[V], q[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s[k] = q[k] = 0.f;
  const uint32_t stride = gridDim.y * BN_BLOCK;
#pragma unroll 4
  for (uint32_t i = blockIdx.y * BN_BLOCK + threadIdx.x; i < g.M;
       i += stride) {
    const VT a = xv[plane_unit(i, c, g)];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float f = to_f(a.v[k]);
      s[k] += f;
      q[k] += f * f;
    }
  }
  plane_block_sum<V>(s, q);
  if (threadIdx.x == 0) {
    float* row = partial + (size_t)blockIdx.y * 2 * g.C;
    row[c] = s[0];
    row[g.C + c] = q[0];
  }
}

template <typename T, int V, int ACT>
BN_KERNEL bn_planes_apply_kernel(const T* __restrict__ x,
                                 const T* __restrict__ z, T* __restrict__ y,
                                 const float* __restrict__ stats,
                                 float* __restrict__ mean_invstd, PlaneGeom g,
                                 ApplyParams p) {
  using VT = Pack<T, V>;
  const uint32_t c = blockIdx.x;
  // the same for the whole block
  const Moments m = moments_of(stats, (int)g.C, (int)c, p.eps);
  const float w = p.w ? ld_param<T>(p.w, p.w_f32, c) : 1.f;
  const float b = p.b ? ld_param<T>(p.b, p.b_f32, c) : 0.f;
  if (blockIdx.y == 0 && threadIdx.x == 0)
    keep_moments<T>(m, (int)g.C, (int)c, mean_invstd, p);
  const VT* xv = reinterpret_cast<const VT*>(x);
  const VT* zv = reinterpret_cast<const VT*>(z);
  VT* yv = reinterpret_cast<VT*>(y);
  const uint32_t stride = gridDim.y * BN_BLOCK;
#pragma unroll 4
  for (uint32_t i = blockIdx.y * BN_BLOCK + threadIdx.x; i < g.M;
       i += stride) {
    const size_t at = plane_unit(i, c, g);
    VT a = xv[at];
    if constexpr (ACT == ACT_NONE) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        a.v[k] = from_f<T>((to_f(a.v[k]) - m.mean) * m.invstd * w + b);
    } else {
      VT res;
      if constexpr (ACT == ACT_ADD_RELU) res = zv[at];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float v = (to_f(a.v[k]) - m.mean) * m.invstd * w + b;
        if constexpr (ACT == ACT_ADD_RELU) v += to_f(res.v[k]);
        a.v[k] = from_f<T>(relu_keep_nan(v));
      }
    }
    yv[at] = a;
  }
}

// MASKED: dy counts only where the forward's output y is above zero
template <typename T, int V, bool MASKED>
BN_KERNEL bn_planes_bwd_reduce_kernel(const T* __restrict__ dy,
                                      const T* __restrict__ x,
                                      const T* __restrict__ y,
                                      const float* __restrict__ mean_invstd,
                                      float* __restrict__ partial,
                                      PlaneGeom g) {
  using VT = Pack<T, V>;
  const uint32_t c = blockIdx.x;
  const float mean = mean_invstd[c];
  const VT* gv = reinterpret_cast<const VT*>(dy);
  const VT* xv = reinterpret_cast<const VT*>(x);
  const VT* yv = reinterpret_cast<const VT*>(y);
  float s1[V], s2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s1[k] = s2[k] = 0.f;
  const uint32_t stride = gridDim.y * BN_BLOCK;
#pragma unroll 2
  for (uint32_t i = blockIdx.y * BN_BLOCK + threadIdx.x; i < g.M;
       i += stride) {
    const size_t at = plane_unit(i, c, g);
    const VT d = gv[at];
    const VT a = xv[at];
    VT o;
    if constexpr (MASKED) o = yv[at];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float f = to_f(d.v[k]);
      if constexpr (MASKED) f = to_f(o.v[k]) > 0.f ? f : 0.f;
      s1[k] += f;
      s2[k] += f * (to_f(a.v[k]) - mean);
    }
  }
  plane_block_sum<V>(s1, s2);
  if (threadIdx.x == 0) {
    float* row = partial + (size_t)blockIdx.y * 2 * g.C;
    row[c] = s1[0];
    row[g.C + c] = s2[0];
  }
}

template <typename T, int V, bool MASKED>
BN_KERNEL bn_planes_bwd_apply_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const T* __restrict__ y,
                                     T* __restrict__ dx, T* __restrict__ dz,
                                     const float* __restrict__ packed,
                                     const float* __restrict__ stats,
                                     const float* __restrict__ mean_invstd,
                                     const void* __restrict__ w, int w_f32,
                                     PlaneGeom g) {
  using VT = Pack<T, V>;
  const uint32_t c = blockIdx.x;
  // the same for the whole block
  const BwdCoef co = bwd_coef<T>(packed, stats, mean_invstd, w, w_f32,
                                 (int)g.C, (int)c);
  const VT* gv = reinterpret_cast<const VT*>(dy);
  const VT* xv = reinterpret_cast<const VT*>(x);
  const VT* yv = reinterpret_cast<const VT*>(y);
  VT* dv = reinterpret_cast<VT*>(dx);
  VT* zv = reinterpret_cast<VT*>(dz);
  const uint32_t stride = gridDim.y * BN_BLOCK;
#pragma unroll 2
  for (uint32_t i = blockIdx.y * BN_BLOCK + threadIdx.x; i < g.M;
       i += stride) {
    const size_t at = plane_unit(i, c, g);
    VT d = gv[at];
    const VT a = xv[at];
    if constexpr (MASKED) {
      const VT o = yv[at];
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (!(to_f(o.v[k]) > 0.f)) d.v[k] = from_f<T>(0.f);
      if (dz) zv[at] = d;
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
      d.v[k] = from_f<T>(
          (to_f(d.v[k]) - co.k1 - (to_f(a.v[k]) - co.mean) * co.k2) *
          co.scale);
    dv[at] = d;
  }
}

// ---------------------------------------------------------------------------
// second stage of both reductions
// ---------------------------------------------------------------------------

// out[c] = sum of column c of the [nrows, 2C] partials and out[C + c] of
// column C + c, rows added in a fixed order: 32 slices per channel keep a
// thread's chain of loads short, their results are added pairwise.
// Forward: out is stats and out[2C] = count. Backward: out is the packed
// vector, and from these local sums gb[c] = out[c] and
// gw[c] = out[C + c] * invstd[c], where wanted.
template <typename T>
BN_KERNEL bn_finalize_kernel(const float* __restrict__ partial, int nrows,
                             int C, float* __restrict__ out, int with_count,
                             float count,
                             const float* __restrict__ mean_invstd,
                             void* __restrict__ gw, int gw_f32,
                             void* __restrict__ gb, int gb_f32) {
  __shared__ float red[2][BN_FIN_SL][BN_FIN_CH];
  const int cl = threadIdx.x % BN_FIN_CH, sl = threadIdx.x / BN_FIN_CH;
  const int c = blockIdx.x * BN_FIN_CH + cl;
  float a = 0.f, b = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int r = sl; r < nrows; r += BN_FIN_SL) {
      a += partial[(size_t)r * 2 * C + c];
      b += partial[(size_t)r * 2 * C + C + c];
    }
  }
  red[0][sl][cl] = a;
  red[1][sl][cl] = b;
  __syncthreads();
  for (int h = BN_FIN_SL / 2; h > 0; h /= 2) {
    if (sl < h) {
      red[0][sl][cl] += red[0][sl + h][cl];
      red[1][sl][cl] += red[1][sl + h][cl];
    }
    __syncthreads();
  }
  if (sl == 0 && c < C) {
    const float ta = red[0][0][cl], tb = red[1][0][cl];
    out[c] = ta;
    out[C + c] = tb;
    if (gb) st_param<T>(gb, gb_f32, c, ta);
    if (gw) st_param<T>(gw, gw_f32, c, tb * mean_invstd[C + c]);
  }
  if (with_count && blockIdx.x == 0 && threadIdx.x == 0) out[2 * C] = count;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

template <typename T> RowsGeom rows_geom(int C) {
  constexpr int V = 16 / sizeof(T);
  RowsGeom g;
  g.C = C;
  g.CVtot = C / V;
  const int tiles = (g.CVtot + BN_BLOCK - 1) / BN_BLOCK;
  g.CVT = (g.CVtot + tiles - 1) / tiles;
  g.RL = BN_BLOCK / g.CVT;
  return g;
}

inline unsigned rows_tiles(const RowsGeom& g) {
  return (unsigned)((g.CVtot + g.CVT - 1) / g.CVT);
}

inline unsigned rows_grid(size_t rows, int RL, size_t cap) {
  size_t blocks = (rows + RL - 1) / RL;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks ? blocks : 1);
}

// row-blocks of the reducing kernels: the [blocks, 2C] f32 partial buffer
// stays at or under 1 MB, or 128 rows
inline size_t rows_reduce_cap(int C) {
  size_t cap = (size_t)131072 / (size_t)C;
  if (cap > 512) cap = 512;
  if (cap < 128) cap = 128;
  return cap;
}

// blocks that share one channel of M load units
inline unsigned plane_splits(size_t M, int C) {
  size_t s = (M + BN_BLOCK * BN_PLANE_LOADS - 1) / (BN_BLOCK * BN_PLANE_LOADS);
  size_t cap = (size_t)BN_PLANE_MAX_BLOCKS / (size_t)C;
  if (cap > BN_PLANE_MAX_SPLITS) cap = BN_PLANE_MAX_SPLITS;
  if (cap < 1) cap = 1;
  if (s > cap) s = cap;
  return (unsigned)(s ? s : 1);
}

template <int V> PlaneGeom plane_geom(size_t N, int C, size_t S) {
  PlaneGeom g;
  g.C = (uint32_t)C;
  g.SV = (uint32_t)(S / V);
  g.M = (uint32_t)(N * (S / V));
  return g;
}

template <typename T>
void finalize_t(const float* partial, unsigned nrows, int C, float* out,
                int with_count, float count, const float* mean_invstd,
                void* gw, int gw_f32, void* gb, int gb_f32,
                hipStream_t stream) {
  hipLaunchKernelGGL((bn_finalize_kernel<T>),
                     dim3((C + BN_FIN_CH - 1) / BN_FIN_CH), dim3(BN_BLOCK), 0,
                     stream, partial, (int)nrows, C, out, with_count, count,
                     mean_invstd, gw, gw_f32, gb, gb_f32);
}

// layout: 0 rows (N counts rows, S == 1), 1 planes with element loads,
// 2 planes with 16-byte loads

template <typename T>
void stats_t(int layout, const void* x, float* partial, float* stats,
             size_t N, int C, size_t S, hipStream_t stream) {
  constexpr int V = 16 / sizeof(T);
  unsigned nrows;
  if (layout == 0) {
    const RowsGeom g = rows_geom<T>(C);
    nrows = rows_grid(N, g.RL, rows_reduce_cap(C));
    hipLaunchKernelGGL((bn_rows_stats_kernel<T>), dim3(nrows, rows_tiles(g)),
                       dim3(BN_BLOCK), 0, stream, (const T*)x, partial, N, g);
  } else if (layout == 1) {
    const PlaneGeom g = plane_geom<1>(N, C, S);
    nrows = plane_splits(g.M, C);
    hipLaunchKernelGGL((bn_planes_stats_kernel<T, 1>), dim3(C, nrows),
                       dim3(BN_BLOCK), 0, stream, (const T*)x, partial, g);
  } else {
    const PlaneGeom g = plane_geom<V>(N, C, S);
    nrows = plane_splits(g.M, C);
    hipLaunchKernelGGL((bn_planes_stats_kernel<T, V>), dim3(C, nrows),
                       dim3(BN_BLOCK), 0, stream, (const T*)x, partial, g);
  }
  finalize_t<T>(partial, nrows, C, stats, 1, (float)(N * S), nullptr, nullptr,
                0, nullptr, 0, stream);
}

// act: ACT_*; z is the residual of ACT_ADD_RELU, mask the rows layout's
// sign bytes of ACT_RELU and ACT_ADD_RELU
template <typename T, int ACT>
void apply_a(int layout, const void* x, const void* z, void* y, void* mask,
             const float* stats, float* mean_invstd, size_t N, int C,
             size_t S, ApplyParams p, hipStream_t stream) {
  constexpr int V = 16 / sizeof(T);
  if (layout == 0) {
    const RowsGeom g = rows_geom<T>(C);
    hipLaunchKernelGGL(
        (bn_rows_apply_kernel<T, ACT>),
        dim3(rows_grid(N, g.RL, BN_APPLY_MAX_GRID), rows_tiles(g)),
        dim3(BN_BLOCK), 0, stream, (const T*)x, (const T*)z, (T*)y,
        (uint8_t*)mask, stats, mean_invstd, N, g, p);
  } else if (layout == 1) {
    const PlaneGeom g = plane_geom<1>(N, C, S);
    hipLaunchKernelGGL((bn_planes_apply_kernel<T, 1, ACT>),
                       dim3(C, plane_splits(g.M, C)), dim3(BN_BLOCK), 0,
                       stream, (const T*)x, (const T*)z, (T*)y, stats,
                       mean_invstd, g, p);
  } else {
    const PlaneGeom g = plane_geom<V>(N, C, S);
    hipLaunchKernelGGL((bn_planes_apply_kernel<T, V, ACT>),
                       dim3(C, plane_splits(g.M, C)), dim3(BN_BLOCK), 0,
                       stream, (const T*)x, (const T*)z, (T*)y, stats,
                       mean_invstd, g, p);
  }
}

template <typename T>
void apply_t(int layout, int act, const void* x, const void* z, void* y,
             void* mask, const float* stats, float* mean_invstd, size_t N,
             int C, size_t S, ApplyParams p, hipStream_t stream) {
  switch (act) {
    case ACT_NONE:
      apply_a<T, ACT_NONE>(layout, x, z, y, mask, stats, mean_invstd, N, C, S,
                           p, stream);
      break;
    case ACT_RELU:
      apply_a<T, ACT_RELU>(layout, x, z, y, mask, stats, mean_invstd, N, C, S,
                           p, stream);
      break;
    case ACT_ADD_RELU:
      apply_a<T, ACT_ADD_RELU>(layout, x, z, y, mask, stats, mean_invstd, N,
                               C, S, p, stream);
      break;
    default:
      throw std::invalid_argument("unknown batch-norm activation code");
  }
}

// saved: what the fused forward kept, the mask bytes (rows) or y (planes)
template <typename T, bool MASKED>
void bwd_reduce_m(int layout, const void* dy, const void* x,
                  const void* saved, const float* mean_invstd, float* partial,
                  float* packed, void* gw, int gw_f32, void* gb, int gb_f32,
                  size_t N, int C, size_t S, hipStream_t stream) {
  constexpr int V = 16 / sizeof(T);
  unsigned nrows;
  if (layout == 0) {
    const RowsGeom g = rows_geom<T>(C);
    nrows = rows_grid(N, g.RL, rows_reduce_cap(C));
    hipLaunchKernelGGL((bn_rows_bwd_reduce_kernel<T, MASKED>),
                       dim3(nrows, rows_tiles(g)), dim3(BN_BLOCK), 0, stream,
                       (const T*)dy, (const T*)x, (const uint8_t*)saved,
                       mean_invstd, partial, N, g);
  } else if (layout == 1) {
    const PlaneGeom g = plane_geom<1>(N, C, S);
    nrows = plane_splits(g.M, C);
    hipLaunchKernelGGL((bn_planes_bwd_reduce_kernel<T, 1, MASKED>),
                       dim3(C, nrows), dim3(BN_BLOCK), 0, stream,
                       (const T*)dy, (const T*)x, (const T*)saved,
                       mean_invstd, partial, g);
  } else {
    const PlaneGeom g = plane_geom<V>(N, C, S);
    nrows = plane_splits(g.M, C);
    hipLaunchKernelGGL((bn_planes_bwd_reduce_kernel<T, V, MASKED>),
                       dim3(C, nrows), dim3(BN_BLOCK), 0, stream,
                       (const T*)dy, (const T*)x, (const T*)saved,
                       mean_invstd, partial, g);
  }
  finalize_t<T>(partial, nrows, C, packed, 0, 0.f, mean_invstd, gw, gw_f32,
                gb, gb_f32, stream);
}

template <typename T>
void bwd_reduce_t(int layout, const void* dy, const void* x,
                  const void* saved, const float* mean_invstd, float* partial,
                  float* packed, void* gw, int gw_f32, void* gb, int gb_f32,
                  size_t N, int C, size_t S, hipStream_t stream) {
  if (saved)
    bwd_reduce_m<T, true>(layout, dy, x, saved, mean_invstd, partial, packed,
                          gw, gw_f32, gb, gb_f32, N, C, S, stream);
  else
    bwd_reduce_m<T, false>(layout, dy, x, saved, mean_invstd, partial, packed,
                           gw, gw_f32, gb, gb_f32, N, C, S, stream);
}

template <typename T, bool MASKED>
void bwd_apply_m(int layout, const void* dy, const void* x, const void* saved,
                 void* dx, void* dz, const float* packed, const float* stats,
                 const float* mean_invstd, const void* w, int w_f32, size_t N,
                 int C, size_t S, hipStream_t stream) {
  constexpr int V = 16 / sizeof(T);
  if (layout == 0) {
    const RowsGeom g = rows_geom<T>(C);
    hipLaunchKernelGGL(
        (bn_rows_bwd_apply_kernel<T, MASKED>),
        dim3(rows_grid(N, g.RL, BN_APPLY_MAX_GRID), rows_tiles(g)),
        dim3(BN_BLOCK), 0, stream, (const T*)dy, (const T*)x,
        (const uint8_t*)saved, (T*)dx, (T*)dz, packed, stats, mean_invstd, w,
        w_f32, N, g);
  } else if (layout == 1) {
    const PlaneGeom g = plane_geom<1>(N, C, S);
    hipLaunchKernelGGL((bn_planes_bwd_apply_kernel<T, 1, MASKED>),
                       dim3(C, plane_splits(g.M, C)), dim3(BN_BLOCK), 0,
                       stream, (const T*)dy, (const T*)x, (const T*)saved,
                       (T*)dx, (T*)dz, packed, stats, mean_invstd, w, w_f32,
                       g);
  } else {
    const PlaneGeom g = plane_geom<V>(N, C, S);
    hipLaunchKernelGGL((bn_planes_bwd_apply_kernel<T, V, MASKED>),
                       dim3(C, plane_splits(g.M, C)), dim3(BN_BLOCK), 0,
                       stream, (const T*)dy, (const T*)x, (const T*)saved,
                       (T*)dx, (T*)dz, packed, stats, mean_invstd, w, w_f32,
                       g);
  }
}

template <typename T>
void bwd_apply_t(int layout, const void* dy, const void* x, const void* saved,
                 void* dx, void* dz, const float* packed, const float* stats,
                 const float* mean_invstd, const void* w, int w_f32, size_t N,
                 int C, size_t S, hipStream_t stream) {
  if (saved)
    bwd_apply_m<T, true>(layout, dy, x, saved, dx, dz, packed, stats,
                         mean_invstd, w, w_f32, N, C, S, stream);
  else
    bwd_apply_m<T, false>(layout, dy, x, saved, dx, dz, packed, stats,
                          mean_invstd, w, w_f32, N, C, S, stream);
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers; what the caller has checked is in launchers.h
// ---------------------------------------------------------------------------

extern "C" {

size_t bagua_bn_partial_rows(int dtype, int layout, size_t N, int C,
                             size_t S) {
  const int V = dtype == BAGUA_F32 ? 4 : 8;
  if (layout == 0) {
    const int CVtot = C / V;
    const int tiles = (CVtot + BN_BLOCK - 1) / BN_BLOCK;
    const int CVT = (CVtot + tiles - 1) / tiles;
    return rows_grid(N, BN_BLOCK / CVT, rows_reduce_cap(C));
  }
  return plane_splits(N * (layout == 2 ? S / V : S), C);
}

void bagua_bn_stats_launch(int dtype, int layout, const void* x,
                           float* partial, float* stats, size_t N, int C,
                           size_t S, hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, stats_t, layout, x, partial, stats, N, C, S,
                 stream);
}

void bagua_bn_apply_launch(int dtype, int layout, int act, const void* x,
                           const void* z, void* y, void* mask,
                           const float* stats, float* mean_invstd,
                           const void* w, int w_f32, const void* b, int b_f32,
                           void* rmean, void* rvar, int r_f32, float momentum,
                           float one_minus_momentum, float eps, size_t N,
                           int C, size_t S, hipStream_t stream) {
  ApplyParams p;
  p.w = w;
  p.b = b;
  p.rmean = rmean;
  p.rvar = rvar;
  p.w_f32 = w_f32;
  p.b_f32 = b_f32;
  p.r_f32 = r_f32;
  p.momentum = momentum;
  p.one_minus_momentum = one_minus_momentum;
  p.eps = eps;
  DISPATCH_DTYPE(dtype, bf16_t, apply_t, layout, act, x, z, y, mask, stats,
                 mean_invstd, N, C, S, p, stream);
}

void bagua_bn_bwd_reduce_launch(int dtype, int layout, const void* dy,
                                const void* x, const void* saved,
                                const float* mean_invstd, float* partial,
                                float* packed, void* gw, int gw_f32, void* gb,
                                int gb_f32, size_t N, int C, size_t S,
                                hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, bwd_reduce_t, layout, dy, x, saved,
                 mean_invstd, partial, packed, gw, gw_f32, gb, gb_f32, N, C,
                 S, stream);
}

void bagua_bn_bwd_apply_launch(int dtype, int layout, const void* dy,
                               const void* x, const void* saved, void* dx,
                               void* dz, const float* packed,
                               const float* stats, const float* mean_invstd,
                               const void* w, int w_f32, size_t N, int C,
                               size_t S, hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, bwd_apply_t, layout, dy, x, saved, dx, dz,
                 packed, stats, mean_invstd, w, w_f32, N, C, S, stream);
}

}  // extern "C"
