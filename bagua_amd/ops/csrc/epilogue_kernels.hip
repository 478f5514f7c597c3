// CDNA4 (gfx950) kernels for the convolution epilogue of a
// Conv2d -> ReLU [-> MaxPool2d(2, 2)] stage, forward and backward.
//
// torch runs this stage as separate memory-bound passes (bias add_, relu_,
// max_pool2d with int64 indices; max_pool2d backward, threshold_backward,
// bias-gradient reduction). Here each direction is one pass:
//
//   bias_relu            y = relu(T(x + b)), in place on the conv output
//   bias_relu_pool       the same, and p = maxpool2x2/s2(y); no indices
//   relu_bwd             dx = y <= 0 ? 0 : g,           db = sum_rows dx
//   pool_relu_bwd        the pool's winner is found again from y; dx gets g
//                        there (if y > 0) and 0 elsewhere, db = sum_rows dx
//
// and the compact pair, for a stage whose y nothing but its own backward
// would read:
//
//   bias_relu_pool_code  p as above and one code byte per pooled element
//                        (the winner's position, and whether it was <= 0);
//                        the conv output is only read
//   pool_code_bwd        pool_relu_bwd from g and the code, without y
//
// Everything but db is bit for bit what the torch chain computes:
//  * x + b is rounded to T before the ReLU (the in-place add_ did that);
//    bf16 rounding is torch's (nearest even, every NaN becomes 0x7FC0);
//  * relu keeps a NaN (clamp_min does), so it is not a plain fmaxf;
//  * the window scan is torch's: h then w from -inf, take the value when
//    `val > max || isnan(val)`: first maximum on ties, the last NaN wins;
//  * max_pool2d backward hands the winner its g unchanged (a -0.0 stays
//    -0.0); threshold_backward then passes it where !(y <= 0).
//
// Layout: channels-last data seen as [rows = N*H*W, C]. A 256-thread block
// is CV = C/V lanes along C (V elements = 16 bytes per lane) times
// RL = 256/CV row-lanes, so a block touches RL whole rows at a time and a
// thread keeps its channels for the whole kernel: bias and the db partial
// sums live in registers. Grids are capped and grid-stride over rows.
//
// db is deterministic, no float atomics: per-thread f32 partial sums, a
// fixed-order LDS reduction over the block's row-lanes into one row of a
// [blocks, C] f32 buffer, and a second kernel that sums the rows in a fixed
// order and rounds once to T.

#include <hip/hip_runtime.h>  // by name in every .hip file: see device_util.h
#include <cmath>

#include "device_util.h"  // to_f / from_f (bf16 is bf16_t), Vec16
#include "launchers.h"

#define EPI_BLOCK 256
#define EPI_MAX_GRID 2048
// finalize: 8 channels x 32 slices of the partial rows per block
#define EPI_FIN_CH 8
#define EPI_FIN_SL (EPI_BLOCK / EPI_FIN_CH)

namespace {

// relu(T(x + b)) as add_ then clamp_min_(0) give it
template <typename T>
__device__ __forceinline__ T bias_relu(T x, float b) {
  const T t = from_f<T>(to_f(x) + b);
  const float f = to_f(t);
  return (f != f) ? t : from_f<T>(fmaxf(f, 0.f));
}

// torch's 2x2 window scan over y[0..3] = (h0w0, h0w1, h1w0, h1w1)
template <typename T>
__device__ __forceinline__ int pool_winner(const T (&y)[4], T& best) {
  float m = -INFINITY;
  int idx = 0;
  best = from_f<T>(m);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float f = to_f(y[k]);
    if (f > m || f != f) {
      m = f;
      best = y[k];
      idx = k;
    }
  }
  return idx;
}

// What pool_relu_bwd needs of a window's four y: the winner's position in
// bits 0..1 and, in bit 2, the backward's own `best <= 0` (false for a NaN).
#define EPI_CODE_DEAD 4

// a lane's N code bytes, stored and loaded as one
template <int N> struct alignas(N) Bytes {
  uint8_t v[N];
};

// A thread's place in the block: channel vector tc, row-lane tr.
struct Lane {
  int tc, tr;
  bool active;
};

__device__ __forceinline__ Lane lane_of(int CV, int RL) {
  Lane l;
  l.tc = threadIdx.x % CV;
  l.tr = threadIdx.x / CV;
  l.active = l.tr < RL;
  return l;
}

template <typename T, int V>
__device__ __forceinline__ void load_bias(const T* __restrict__ bias, int tc,
                                          float (&b)[V]) {
  // element loads: a bias that is a view into a flat parameter buffer need
  // not be 16-byte aligned
#pragma unroll
  for (int q = 0; q < V; ++q) b[q] = to_f(bias[tc * V + q]);
}

// Sum the row-lanes' partials in lane order and store the block's row of
// the partial buffer. Every thread of the block must call this.
template <int V>
__device__ __forceinline__ void block_reduce_store(
    const float (&acc)[V], const Lane& l, int CV, int RL,
    float* __restrict__ partial_row) {
  __shared__ float red[EPI_BLOCK * V];
  const int C = CV * V;
  if (l.active) {
#pragma unroll
    for (int q = 0; q < V; ++q) red[l.tr * C + l.tc * V + q] = acc[q];
  }
  __syncthreads();
  for (int j = threadIdx.x; j < C; j += EPI_BLOCK) {
    float s = 0.f;
    for (int t = 0; t < RL; ++t) s += red[t * C + j];
    partial_row[j] = s;
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

template <typename T, int U>
__global__ void __launch_bounds__(EPI_BLOCK)
epi_bias_relu_kernel(T* __restrict__ x, const T* __restrict__ bias,
                     size_t rows, int CV, int RL) {
  using VT = Vec16<T>;
  constexpr int V = VT::N;
  const Lane l = lane_of(CV, RL);
  if (!l.active) return;
  float b[V];
  load_bias<T, V>(bias, l.tc, b);
  VT* xv = reinterpret_cast<VT*>(x) + l.tc;
  const size_t stride = (size_t)gridDim.x * RL;
  size_t r = (size_t)blockIdx.x * RL + l.tr;
  for (; r + (U - 1) * stride < rows; r += U * stride) {
    VT a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = xv[(r + u * stride) * CV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int q = 0; q < V; ++q) a[u].v[q] = bias_relu(a[u].v[q], b[q]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xv[(r + u * stride) * CV] = a[u];
  }
  for (; r < rows; r += stride) {
    VT a = xv[r * CV];
#pragma unroll
    for (int q = 0; q < V; ++q) a.v[q] = bias_relu(a.v[q], b[q]);
    xv[r * CV] = a;
  }
}

// Input rows of pooled row o (W = 2*Wo, H even): with q = o / Wo = n*Ho + oh
// and ow = o % Wo the window starts at row 2*q*W + 2*ow.
__device__ __forceinline__ void window_rows(size_t o, uint32_t Wo,
                                            size_t (&r)[4]) {
  const size_t q = (uint32_t)o / Wo;
  const size_t ow = o - q * Wo;
  const size_t W = 2 * (size_t)Wo;
  r[0] = 2 * q * W + 2 * ow;
  r[1] = r[0] + 1;
  r[2] = r[0] + W;
  r[3] = r[2] + 1;
}

template <typename T>
__global__ void __launch_bounds__(EPI_BLOCK)
epi_bias_relu_pool_kernel(T* __restrict__ x, const T* __restrict__ bias,
                          T* __restrict__ p, size_t orows, uint32_t Wo,
                          int CV, int RL) {
  using VT = Vec16<T>;
  constexpr int V = VT::N;
  const Lane l = lane_of(CV, RL);
  if (!l.active) return;
  float b[V];
  load_bias<T, V>(bias, l.tc, b);
  VT* xv = reinterpret_cast<VT*>(x) + l.tc;
  VT* pv = reinterpret_cast<VT*>(p) + l.tc;
  const size_t stride = (size_t)gridDim.x * RL;
  for (size_t o = (size_t)blockIdx.x * RL + l.tr; o < orows; o += stride) {
    size_t r[4];
    window_rows(o, Wo, r);
    VT a[4], out;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = xv[r[k] * CV];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      T y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        y[k] = bias_relu(a[k].v[q], b[q]);
        a[k].v[q] = y[k];
      }
      pool_winner(y, out.v[q]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[r[k] * CV] = a[k];
    pv[o * CV] = out;
  }
}

// The same window walk; y is formed in registers only and x is not written.
// code is [orows, C] bytes.
template <typename T>
__global__ void __launch_bounds__(EPI_BLOCK) NO_PACKED_F32
epi_bias_relu_pool_code_kernel(const T* __restrict__ x,
                               const T* __restrict__ bias, T* __restrict__ p,
                               uint8_t* __restrict__ code, size_t orows,
                               uint32_t Wo, int CV, int RL) {
  using VT = Vec16<T>;
  constexpr int V = VT::N;
  const Lane l = lane_of(CV, RL);
  if (!l.active) return;
  float b[V];
  load_bias<T, V>(bias, l.tc, b);
  const VT* xv = reinterpret_cast<const VT*>(x) + l.tc;
  VT* pv = reinterpret_cast<VT*>(p) + l.tc;
  Bytes<V>* cv = reinterpret_cast<Bytes<V>*>(code) + l.tc;
  const size_t stride = (size_t)gridDim.x * RL;
  for (size_t o = (size_t)blockIdx.x * RL + l.tr; o < orows; o += stride) {
    size_t r[4];
    window_rows(o, Wo, r);
    VT a[4], out;
    Bytes<V> cd;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = xv[r[k] * CV];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      T y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] = bias_relu(a[k].v[q], b[q]);
      const int idx = pool_winner(y, out.v[q]);
      cd.v[q] = (uint8_t)(idx | (to_f(out.v[q]) <= 0.f ? EPI_CODE_DEAD : 0));
    }
    pv[o * CV] = out;
    cv[o * CV] = cd;
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

template <typename T, int U>
__global__ void __launch_bounds__(EPI_BLOCK)
epi_relu_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y,
                    T* __restrict__ dx, float* __restrict__ partial,
                    size_t rows, int CV, int RL) {
  using VT = Vec16<T>;
  constexpr int V = VT::N;
  const Lane l = lane_of(CV, RL);
  float acc[V];
#pragma unroll
  for (int q = 0; q < V; ++q) acc[q] = 0.f;
  if (l.active) {
    const VT* gv = reinterpret_cast<const VT*>(g) + l.tc;
    const VT* yv = reinterpret_cast<const VT*>(y) + l.tc;
    VT* dv = reinterpret_cast<VT*>(dx) + l.tc;
    const T zero = from_f<T>(0.f);
    const size_t stride = (size_t)gridDim.x * RL;
    size_t r = (size_t)blockIdx.x * RL + l.tr;
    for (; r + (U - 1) * stride < rows; r += U * stride) {
      VT a[U], m[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[u] = gv[(r + u * stride) * CV];
        m[u] = yv[(r + u * stride) * CV];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int q = 0; q < V; ++q) {
          if (to_f(m[u].v[q]) <= 0.f) a[u].v[q] = zero;
          acc[q] += to_f(a[u].v[q]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) dv[(r + u * stride) * CV] = a[u];
    }
    for (; r < rows; r += stride) {
      VT a = gv[r * CV];
      const VT m = yv[r * CV];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        if (to_f(m.v[q]) <= 0.f) a.v[q] = zero;
        acc[q] += to_f(a.v[q]);
      }
      dv[r * CV] = a;
    }
  }
  if (partial)
    block_reduce_store<V>(acc, l, CV, RL,
                          partial + (size_t)blockIdx.x * CV * V);
}

template <typename T>
__global__ void __launch_bounds__(EPI_BLOCK)
epi_pool_relu_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y,
                         T* __restrict__ dx, float* __restrict__ partial,
                         size_t orows, uint32_t Wo, int CV, int RL) {
  using VT = Vec16<T>;
  constexpr int V = VT::N;
  const Lane l = lane_of(CV, RL);
  float acc[V];
#pragma unroll
  for (int q = 0; q < V; ++q) acc[q] = 0.f;
  if (l.active) {
    const VT* gv = reinterpret_cast<const VT*>(g) + l.tc;
    const VT* yv = reinterpret_cast<const VT*>(y) + l.tc;
    VT* dv = reinterpret_cast<VT*>(dx) + l.tc;
    const T zero = from_f<T>(0.f);
    const size_t stride = (size_t)gridDim.x * RL;
    for (size_t o = (size_t)blockIdx.x * RL + l.tr; o < orows; o += stride) {
      size_t r[4];
      window_rows(o, Wo, r);
      const VT gg = gv[o * CV];
      VT a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = yv[r[k] * CV];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        T w[4], best;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = a[k].v[q];
        const int idx = pool_winner(w, best);
        T d = gg.v[q];  // as it is, -0.0 included
        if (to_f(best) <= 0.f) d = zero;
        acc[q] += to_f(d);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k].v[q] = (k == idx) ? d : zero;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) dv[r[k] * CV] = a[k];
    }
  }
  if (partial)
    block_reduce_store<V>(acc, l, CV, RL,
                          partial + (size_t)blockIdx.x * CV * V);
}

// epi_pool_relu_bwd_kernel with the winner and its sign read from the code:
// the same rows per thread and the same order of additions, so db has the
// same bits.
template <typename T>
__global__ void __launch_bounds__(EPI_BLOCK) NO_PACKED_F32
epi_pool_code_bwd_kernel(const T* __restrict__ g,
                         const uint8_t* __restrict__ code, T* __restrict__ dx,
                         float* __restrict__ partial, size_t orows,
                         uint32_t Wo, int CV, int RL) {
  using VT = Vec16<T>;
  constexpr int V = VT::N;
  const Lane l = lane_of(CV, RL);
  float acc[V];
#pragma unroll
  for (int q = 0; q < V; ++q) acc[q] = 0.f;
  if (l.active) {
    const VT* gv = reinterpret_cast<const VT*>(g) + l.tc;
    const Bytes<V>* cv = reinterpret_cast<const Bytes<V>*>(code) + l.tc;
    VT* dv = reinterpret_cast<VT*>(dx) + l.tc;
    const T zero = from_f<T>(0.f);
    const size_t stride = (size_t)gridDim.x * RL;
    for (size_t o = (size_t)blockIdx.x * RL + l.tr; o < orows; o += stride) {
      size_t r[4];
      window_rows(o, Wo, r);
      const VT gg = gv[o * CV];
      const Bytes<V> cd = cv[o * CV];
      VT a[4];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const int idx = cd.v[q] & 3;
        T d = gg.v[q];  // as it is, -0.0 included
        if (cd.v[q] & EPI_CODE_DEAD) d = zero;
        acc[q] += to_f(d);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k].v[q] = (k == idx) ? d : zero;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) dv[r[k] * CV] = a[k];
    }
  }
  if (partial)
    block_reduce_store<V>(acc, l, CV, RL,
                          partial + (size_t)blockIdx.x * CV * V);
}

// db[c] = T(sum over the partial rows, in a fixed order). The buffer is a
// few hundred KB and the kernel is latency-bound: many slices per channel
// keep each thread's chain of loads short (16 for 512 rows).
template <typename T>
__global__ void __launch_bounds__(EPI_BLOCK)
epi_bias_grad_finalize_kernel(const float* __restrict__ partial, int nrows,
                              int C, T* __restrict__ db) {
  __shared__ float red[EPI_FIN_SL][EPI_FIN_CH];
  const int cl = threadIdx.x % EPI_FIN_CH, sl = threadIdx.x / EPI_FIN_CH;
  const int c = blockIdx.x * EPI_FIN_CH + cl;
  float s = 0.f;
  if (c < C) {
#pragma unroll 8
    for (int b = sl; b < nrows; b += EPI_FIN_SL)
      s += partial[(size_t)b * C + c];
  }
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < EPI_FIN_SL; ++k) t += red[k][cl];
    db[c] = from_f<T>(t);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

struct Shape {
  int CV, RL;
};

template <typename T> Shape shape_of(int C) {
  Shape s;
  s.CV = C / Vec16<T>::N;
  s.RL = EPI_BLOCK / s.CV;
  return s;
}

inline unsigned grid_for(size_t work_rows, int RL, size_t cap) {
  size_t blocks = (work_rows + RL - 1) / RL;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks ? blocks : 1);
}

// the reducing kernels keep the [blocks, C] f32 partial buffer at or under
// 512 KB
inline size_t reduce_cap(int C) {
  size_t cap = (size_t)131072 / (size_t)C;
  if (cap > 512) cap = 512;
  if (cap < 128) cap = 128;
  return cap;
}

template <typename T>
void bias_relu_t(void* x, const void* bias, size_t rows, int C,
                 hipStream_t stream) {
  const Shape s = shape_of<T>(C);
  hipLaunchKernelGGL((epi_bias_relu_kernel<T, 4>),
                     dim3(grid_for(rows, s.RL, EPI_MAX_GRID)),
                     dim3(EPI_BLOCK), 0, stream, (T*)x, (const T*)bias, rows,
                     s.CV, s.RL);
}

template <typename T>
void bias_relu_pool_t(void* x, const void* bias, void* p, size_t orows,
                      int Wo, int C, hipStream_t stream) {
  const Shape s = shape_of<T>(C);
  hipLaunchKernelGGL((epi_bias_relu_pool_kernel<T>),
                     dim3(grid_for(orows, s.RL, EPI_MAX_GRID)),
                     dim3(EPI_BLOCK), 0, stream, (T*)x, (const T*)bias,
                     (T*)p, orows, (uint32_t)Wo, s.CV, s.RL);
}

template <typename T>
void finalize_t(const float* partial, int nrows, int C, void* db,
                hipStream_t stream) {
  hipLaunchKernelGGL((epi_bias_grad_finalize_kernel<T>),
                     dim3((C + EPI_FIN_CH - 1) / EPI_FIN_CH),
                     dim3(EPI_BLOCK), 0, stream, partial, nrows, C, (T*)db);
}

template <typename T>
void relu_bwd_t(const void* g, const void* y, void* dx, float* partial,
                void* db, size_t rows, int C, hipStream_t stream) {
  const Shape s = shape_of<T>(C);
  const unsigned grid = grid_for(rows, s.RL, reduce_cap(C));
  hipLaunchKernelGGL((epi_relu_bwd_kernel<T, 4>), dim3(grid),
                     dim3(EPI_BLOCK), 0, stream, (const T*)g, (const T*)y,
                     (T*)dx, partial, rows, s.CV, s.RL);
  if (partial) finalize_t<T>(partial, (int)grid, C, db, stream);
}

template <typename T>
void pool_relu_bwd_t(const void* g, const void* y, void* dx, float* partial,
                     void* db, size_t orows, int Wo, int C,
                     hipStream_t stream) {
  const Shape s = shape_of<T>(C);
  const unsigned grid = grid_for(orows, s.RL, reduce_cap(C));
  hipLaunchKernelGGL((epi_pool_relu_bwd_kernel<T>), dim3(grid),
                     dim3(EPI_BLOCK), 0, stream, (const T*)g, (const T*)y,
                     (T*)dx, partial, orows, (uint32_t)Wo, s.CV, s.RL);
  if (partial) finalize_t<T>(partial, (int)grid, C, db, stream);
}

template <typename T>
void bias_relu_pool_code_t(const void* x, const void* bias, void* p,
                           uint8_t* code, size_t orows, int Wo, int C,
                           hipStream_t stream) {
  const Shape s = shape_of<T>(C);
  hipLaunchKernelGGL((epi_bias_relu_pool_code_kernel<T>),
                     dim3(grid_for(orows, s.RL, EPI_MAX_GRID)),
                     dim3(EPI_BLOCK), 0, stream, (const T*)x, (const T*)bias,
                     (T*)p, code, orows, (uint32_t)Wo, s.CV, s.RL);
}

template <typename T>
void pool_code_bwd_t(const void* g, const uint8_t* code, void* dx,
                     float* partial, void* db, size_t orows, int Wo, int C,
                     hipStream_t stream) {
  const Shape s = shape_of<T>(C);
  const unsigned grid = grid_for(orows, s.RL, reduce_cap(C));
  hipLaunchKernelGGL((epi_pool_code_bwd_kernel<T>), dim3(grid),
                     dim3(EPI_BLOCK), 0, stream, (const T*)g, code, (T*)dx,
                     partial, orows, (uint32_t)Wo, s.CV, s.RL);
  if (partial) finalize_t<T>(partial, (int)grid, C, db, stream);
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers; what the caller has checked is in launchers.h
// ---------------------------------------------------------------------------

extern "C" {

size_t bagua_epi_partial_rows(int dtype, size_t work_rows, int C) {
  const int V = dtype == BAGUA_F32 ? 4 : 8;
  return grid_for(work_rows, EPI_BLOCK / (C / V), reduce_cap(C));
}

void bagua_epi_bias_relu_launch(int dtype, void* x, const void* bias,
                                size_t rows, int C, hipStream_t stream) {
  if (rows == 0) return;
  DISPATCH_DTYPE(dtype, bf16_t, bias_relu_t, x, bias, rows, C, stream);
}

void bagua_epi_bias_relu_pool_launch(int dtype, void* x, const void* bias,
                                     void* p, size_t orows, int Wo, int C,
                                     hipStream_t stream) {
  if (orows == 0) return;
  DISPATCH_DTYPE(dtype, bf16_t, bias_relu_pool_t, x, bias, p, orows, Wo, C,
                 stream);
}

void bagua_epi_relu_bwd_launch(int dtype, const void* g, const void* y,
                               void* dx, float* partial, void* db,
                               size_t rows, int C, hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, relu_bwd_t, g, y, dx, partial, db, rows, C,
                 stream);
}

void bagua_epi_pool_relu_bwd_launch(int dtype, const void* g, const void* y,
                                    void* dx, float* partial, void* db,
                                    size_t orows, int Wo, int C,
                                    hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, pool_relu_bwd_t, g, y, dx, partial, db, orows,
                 Wo, C, stream);
}

void bagua_epi_bias_relu_pool_code_launch(int dtype, const void* x,
                                          const void* bias, void* p,
                                          uint8_t* code, size_t orows, int Wo,
                                          int C, hipStream_t stream) {
  if (orows == 0) return;
  DISPATCH_DTYPE(dtype, bf16_t, bias_relu_pool_code_t, x, bias, p, code,
                 orows, Wo, C, stream);
}

void bagua_epi_pool_code_bwd_launch(int dtype, const void* g,
                                    const uint8_t* code, void* dx,
                                    float* partial, void* db, size_t orows,
                                    int Wo, int C, hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, pool_code_bwd_t, g, code, dx, partial, db,
                 orows, Wo, C, stream);
}

}  // extern "C"
