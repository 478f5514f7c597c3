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

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstdint>

#define EPI_BLOCK 256
#define EPI_MAX_GRID 2048
// finalize: 8 channels x 32 slices of the partial rows per block
#define EPI_FIN_CH 8
#define EPI_FIN_SL (EPI_BLOCK / EPI_FIN_CH)

namespace {

struct bf16_t {
  uint16_t bits;
};

template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<__half>(__half v) {
  return __half2float(v);
}
template <> __device__ __forceinline__ float to_f<bf16_t>(bf16_t v) {
  return __uint_as_float((uint32_t)v.bits << 16);
}

template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f<__half>(float v) {
  return __float2half(v);
}
// torch's rounding (c10 round_to_nearest_even), NaN payload included
template <> __device__ __forceinline__ bf16_t from_f<bf16_t>(float v) {
  bf16_t r;
  if (v != v) {
    r.bits = 0x7FC0;
  } else {
    const uint32_t u = __float_as_uint(v);
    r.bits = (uint16_t)((u + ((u >> 16) & 1u) + 0x7FFFu) >> 16);
  }
  return r;
}

template <typename T> struct alignas(16) Vec16 {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

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

}  // namespace

// ---------------------------------------------------------------------------
// launchers (dtype: 0=f32 1=f16 2=bf16). The caller has checked: C is a
// multiple of the 16-byte vector and C / vector <= 256, full-size rows are
// below 2^31, data pointers are 16-byte aligned, H and W are even when
// pooling. `rows` counts full-size rows, `orows` pooled ones.
// ---------------------------------------------------------------------------

#define EPI_DISPATCH(dtype, fn, ...)                                       \
  do {                                                                     \
    if ((dtype) == 0)                                                      \
      fn<float>(__VA_ARGS__);                                              \
    else if ((dtype) == 1)                                                 \
      fn<__half>(__VA_ARGS__);                                             \
    else                                                                   \
      fn<bf16_t>(__VA_ARGS__);                                             \
  } while (0)

extern "C" {

// rows of the f32 partial buffer [blocks, C] the backward launchers need;
// work_rows is `rows` without pooling and `orows` with it
size_t bagua_epi_partial_rows(int dtype, size_t work_rows, int C) {
  const int V = dtype == 0 ? 4 : 8;
  return grid_for(work_rows, EPI_BLOCK / (C / V), reduce_cap(C));
}

void bagua_epi_bias_relu_launch(int dtype, void* x, const void* bias,
                                size_t rows, int C, hipStream_t stream) {
  if (rows == 0) return;
  EPI_DISPATCH(dtype, bias_relu_t, x, bias, rows, C, stream);
}

void bagua_epi_bias_relu_pool_launch(int dtype, void* x, const void* bias,
                                     void* p, size_t orows, int Wo, int C,
                                     hipStream_t stream) {
  if (orows == 0) return;
  EPI_DISPATCH(dtype, bias_relu_pool_t, x, bias, p, orows, Wo, C, stream);
}

// partial == nullptr: dx only, db is left alone
void bagua_epi_relu_bwd_launch(int dtype, const void* g, const void* y,
                               void* dx, float* partial, void* db,
                               size_t rows, int C, hipStream_t stream) {
  EPI_DISPATCH(dtype, relu_bwd_t, g, y, dx, partial, db, rows, C, stream);
}

void bagua_epi_pool_relu_bwd_launch(int dtype, const void* g, const void* y,
                                    void* dx, float* partial, void* db,
                                    size_t orows, int Wo, int C,
                                    hipStream_t stream) {
  EPI_DISPATCH(dtype, pool_relu_bwd_t, g, y, dx, partial, db, orows, Wo, C,
               stream);
}

}  // extern "C"
