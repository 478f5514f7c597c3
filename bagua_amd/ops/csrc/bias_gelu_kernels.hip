// CDNA4 (gfx950) kernels for the middle of a transformer MLP, the activation
// behind its first Linear, forward and backward, over rows [R, C]:
//
//   z = f32(h) + f32(bias)         a = T(gelu(z))
//   dz = f32(dy) * gelu'(z)        dh = T(dz)       db = sum over rows of dz
//
// h is the Linear's output without its bias. Backward forms z again from h
// and bias, so h is all that has to be kept. gelu is the erf form or the
// tanh form, with the constants of torch.nn.functional.gelu.
//
//   bg_fwd           a row is cut into chunks of 8 elements (16 bytes of a
//                    2-byte type, two 16-byte vectors of f32) and the chunks
//                    into column tiles of BAGUA_BG_TILE_CHUNKS; blockIdx.x is
//                    the tile, so a row may be as long as it likes. In a
//                    block, lane (threadIdx.x % CL) takes one chunk of the
//                    tile and threadIdx.x / CL picks the row; CL is 64, a
//                    whole wave along the row, or for rows of fewer chunks
//                    the next power of two, and then a wave covers several
//                    rows. blockIdx.y grid-strides over rows under a capped
//                    grid. A thread keeps its columns for the whole kernel:
//                    its 8 bias values are loaded once. It works on two rows
//                    at a time, a stride of the grid apart, so that four
//                    (backward: eight) 16-byte loads are in flight per lane.
//   bg_bwd           the same shape. The thread's 8 db partials are f32
//                    registers over all its rows, added in row order. At the
//                    end the block's rows are added through 8 KB of LDS in a
//                    fixed order into the block's row of an f32 buffer
//                    [gridDim.y, C].
//   bg_bwd_finalize  adds those rows in a fixed order and writes db, rounded
//                    once, in its parameter's dtype.
//
// Without a bias (null) this is plain GELU and no db work happens. erf or
// tanh is a template parameter: a kernel then holds the code and the
// registers of one form only. All arithmetic is f32 with one rounding per
// stored value (bf16 as torch rounds). No atomics: every sum has a fixed
// order, so results are the same bits from run to run.

#include <hip/hip_runtime.h>  // by name in every .hip file: see device_util.h
#include <cmath>

#include "device_util.h"  // to_f / from_f (bf16 is bf16_t), Vec16
#include "launchers.h"

#define BG_BLOCK BAGUA_BG_BLOCK
#define BG_TILE BAGUA_BG_TILE_CHUNKS
// finalize: 16 columns x 16 slices of the partial rows per block
#define BG_FIN_COLS 16
#define BG_FIN_SL (BG_BLOCK / BG_FIN_COLS)

#define BG_KERNEL \
  __global__ void __launch_bounds__(BG_BLOCK) NO_PACKED_F32

namespace {

// bias and db are f32 or T, told at run time; element access, as they may be
// views into a flat parameter buffer and need not be aligned
template <typename T>
__device__ __forceinline__ float ld_param(const void* p, int is_f32,
                                          size_t i) {
  return is_f32 ? static_cast<const float*>(p)[i]
                : to_f(static_cast<const T*>(p)[i]);
}

// a chunk: 8 elements from a 16-byte aligned p, as f32
template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
  constexpr int N = Vec16<T>::N;  // 4 or 8
  const Vec16<T>* v = reinterpret_cast<const Vec16<T>*>(p);
#pragma unroll
  for (int q = 0; q < 8 / N; ++q) {
    const Vec16<T> a = v[q];
#pragma unroll
    for (int k = 0; k < N; ++k) f[q * N + k] = to_f(a.v[k]);
  }
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&f)[8]) {
  constexpr int N = Vec16<T>::N;
  Vec16<T>* v = reinterpret_cast<Vec16<T>*>(p);
#pragma unroll
  for (int q = 0; q < 8 / N; ++q) {
    Vec16<T> a;
#pragma unroll
    for (int k = 0; k < N; ++k) a.v[k] = from_f<T>(f[q * N + k]);
    v[q] = a;
  }
}

// torch's constants (ATen/native/cuda/ActivationGeluKernel.cu), as it forms
// them: in double, cast once
constexpr float kSqrtHalf = (float)M_SQRT1_2;
constexpr float kErfPdf = (float)(M_2_SQRTPI * M_SQRT1_2 * 0.5);
constexpr float kTanhBeta = (float)(M_SQRT2 * M_2_SQRTPI * 0.5);
constexpr float kTanhKappa = 0.044715f;

template <bool TANH>
__device__ __forceinline__ float gelu(float z) {
  if constexpr (TANH) {
    const float inner = kTanhBeta * (z + kTanhKappa * z * z * z);
    return 0.5f * z * (1.f + tanhf(inner));
  } else {
    return 0.5f * z * (1.f + erff(z * kSqrtHalf));
  }
}

// d gelu / dz
template <bool TANH>
__device__ __forceinline__ float gelu_grad(float z) {
  if constexpr (TANH) {
    const float z2 = z * z;
    const float t = tanhf(kTanhBeta * (z + kTanhKappa * z2 * z));
    const float inner_d = kTanhBeta * (1.f + 3.f * kTanhKappa * z2);
    return 0.5f * (1.f + t) + 0.5f * z * ((1.f - t * t) * inner_d);
  } else {
    const float cdf = 0.5f * (1.f + erff(z * kSqrtHalf));
    const float pdf = expf(-0.5f * z * z) * kErfPdf;
    return cdf + z * pdf;
  }
}

// Where a thread stands: its chunk's first column (valid below C), its
// first row and the rows between two of its visits. cshift is log2(CL).
struct Place {
  size_t col, row, stride;
};
__device__ __forceinline__ Place place(int cshift) {
  Place p;
  const unsigned cl = threadIdx.x & ((1u << cshift) - 1u);
  const unsigned rl = threadIdx.x >> cshift, rb = BG_BLOCK >> cshift;
  p.col = ((size_t)blockIdx.x * BG_TILE + cl) * 8;
  p.row = (size_t)blockIdx.y * rb + rl;
  p.stride = (size_t)gridDim.y * rb;
  return p;
}

template <typename T, bool TANH>
BG_KERNEL bg_fwd_kernel(const T* __restrict__ h, const void* __restrict__ bias,
                        int bias_f32, T* __restrict__ a, size_t R, size_t C,
                        int cshift) {
  const Place p = place(cshift);
  if (p.col >= C) return;  // no barrier below
  float b[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    b[k] = bias ? ld_param<T>(bias, bias_f32, p.col + k) : 0.f;

  for (size_t r0 = p.row; r0 < R; r0 += 2 * p.stride) {
    const size_t r1 = r0 + p.stride;
    const bool two = r1 < R;
    const size_t e0 = r0 * C + p.col, e1 = r1 * C + p.col;
    float z0[8], z1[8];
    load8<T>(h + e0, z0);
    if (two) load8<T>(h + e1, z1);
#pragma unroll
    for (int k = 0; k < 8; ++k) z0[k] = gelu<TANH>(z0[k] + b[k]);
    store8<T>(a + e0, z0);
    if (two) {
#pragma unroll
      for (int k = 0; k < 8; ++k) z1[k] = gelu<TANH>(z1[k] + b[k]);
      store8<T>(a + e1, z1);
    }
  }
}

// partial == nullptr: dh only
template <typename T, bool TANH>
BG_KERNEL bg_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h,
                        const void* __restrict__ bias, int bias_f32,
                        T* __restrict__ dh, float* __restrict__ partial,
                        size_t R, size_t C, int cshift) {
  __shared__ float red[BG_BLOCK * 8];  // [rows of the block][CL * 8]
  const Place p = place(cshift);
  const bool live = p.col < C;
  float b[8], acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    b[k] = (bias && live) ? ld_param<T>(bias, bias_f32, p.col + k) : 0.f;
    acc[k] = 0.f;
  }

  if (live) {
    for (size_t r0 = p.row; r0 < R; r0 += 2 * p.stride) {
      const size_t r1 = r0 + p.stride;
      const bool two = r1 < R;
      const size_t e0 = r0 * C + p.col, e1 = r1 * C + p.col;
      float z0[8], g0[8], z1[8], g1[8];
      load8<T>(h + e0, z0);
      load8<T>(dy + e0, g0);
      if (two) {
        load8<T>(h + e1, z1);
        load8<T>(dy + e1, g1);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        g0[k] *= gelu_grad<TANH>(z0[k] + b[k]);
        acc[k] += g0[k];
      }
      store8<T>(dh + e0, g0);
      if (two) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          g1[k] *= gelu_grad<TANH>(z1[k] + b[k]);
          acc[k] += g1[k];
        }
        store8<T>(dh + e1, g1);
      }
    }
  }

  if (!partial) return;  // the whole grid
  // the block's rows of each column, added in row order
  const int width = 8 << cshift, rb = BG_BLOCK >> cshift;
#pragma unroll
  for (int k = 0; k < 8; ++k) red[threadIdx.x * 8 + k] = acc[k];
  __syncthreads();
  for (int idx = threadIdx.x; idx < width; idx += BG_BLOCK) {
    const size_t c = (size_t)blockIdx.x * BG_TILE * 8 + idx;
    if (c < C) {
      float t = red[idx];
      for (int rl = 1; rl < rb; ++rl) t += red[rl * width + idx];
      partial[(size_t)blockIdx.y * C + c] = t;
    }
  }
}

// Column c of the [nrows, C] partials, rows added in a fixed order: 16
// slices per column keep a thread's chain of loads short, their results are
// added pairwise.
template <typename T>
BG_KERNEL bg_bwd_finalize_kernel(const float* __restrict__ partial, int nrows,
                                 size_t C, void* db, int db_f32) {
  __shared__ float red[BG_FIN_SL][BG_FIN_COLS];
  const int cl = threadIdx.x % BG_FIN_COLS, sl = threadIdx.x / BG_FIN_COLS;
  const size_t c = (size_t)blockIdx.x * BG_FIN_COLS + cl;
  float t = 0.f;
  if (c < C) {
#pragma unroll 4
    for (int r = sl; r < nrows; r += BG_FIN_SL) t += partial[(size_t)r * C + c];
  }
  red[sl][cl] = t;
  __syncthreads();
  for (int half = BG_FIN_SL / 2; half > 0; half /= 2) {
    if (sl < half) red[sl][cl] += red[sl + half][cl];
    __syncthreads();
  }
  if (sl == 0 && c < C) {
    if (db_f32)
      static_cast<float*>(db)[c] = red[0][cl];
    else
      static_cast<T*>(db)[c] = from_f<T>(red[0][cl]);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// log2 of the lanes along a row: 64 lanes from 64 chunks on, else the next
// power of two at or above the row's chunks
inline int col_shift(size_t C) {
  int s = 0;
  while (s < 6 && ((size_t)8 << s) < C) ++s;
  return s;
}

inline size_t col_tiles(size_t C) {
  return (C / 8 + BG_TILE - 1) / BG_TILE;
}

// gridDim.y. With db it is also the rows of the partial buffer, which stays
// within BAGUA_BG_PARTIAL_BYTES or, for a row longer than that, is one row.
inline unsigned row_blocks(size_t R, size_t C, bool with_db) {
  const size_t rb = BG_BLOCK >> col_shift(C);
  size_t blocks = (R + rb - 1) / rb;
  size_t cap = BAGUA_BG_MAX_GRID / col_tiles(C);
  if (with_db && cap > BAGUA_BG_PARTIAL_BYTES / 4 / C)
    cap = BAGUA_BG_PARTIAL_BYTES / 4 / C;
  if (cap < 1) cap = 1;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks ? blocks : 1);
}

template <typename T, bool TANH>
void fwd_f(const void* h, const void* bias, int bias_f32, void* a, size_t R,
           size_t C, hipStream_t stream) {
  hipLaunchKernelGGL((bg_fwd_kernel<T, TANH>),
                     dim3((unsigned)col_tiles(C), row_blocks(R, C, false)),
                     dim3(BG_BLOCK), 0, stream, (const T*)h, bias, bias_f32,
                     (T*)a, R, C, col_shift(C));
}
template <typename T>
void fwd_t(int tanh_form, const void* h, const void* bias, int bias_f32,
           void* a, size_t R, size_t C, hipStream_t stream) {
  if (tanh_form)
    fwd_f<T, true>(h, bias, bias_f32, a, R, C, stream);
  else
    fwd_f<T, false>(h, bias, bias_f32, a, R, C, stream);
}

template <typename T, bool TANH>
void bwd_f(const void* dy, const void* h, const void* bias, int bias_f32,
           void* dh, float* partial, void* db, int db_f32, size_t R, size_t C,
           hipStream_t stream) {
  const unsigned rows = row_blocks(R, C, partial != nullptr);
  hipLaunchKernelGGL((bg_bwd_kernel<T, TANH>),
                     dim3((unsigned)col_tiles(C), rows), dim3(BG_BLOCK), 0,
                     stream, (const T*)dy, (const T*)h, bias, bias_f32,
                     (T*)dh, partial, R, C, col_shift(C));
  if (!partial) return;
  hipLaunchKernelGGL(
      (bg_bwd_finalize_kernel<T>),
      dim3((unsigned)((C + BG_FIN_COLS - 1) / BG_FIN_COLS)), dim3(BG_BLOCK),
      0, stream, partial, (int)rows, C, db, db_f32);
}
template <typename T>
void bwd_t(int tanh_form, const void* dy, const void* h, const void* bias,
           int bias_f32, void* dh, float* partial, void* db, int db_f32,
           size_t R, size_t C, hipStream_t stream) {
  if (tanh_form)
    bwd_f<T, true>(dy, h, bias, bias_f32, dh, partial, db, db_f32, R, C,
                   stream);
  else
    bwd_f<T, false>(dy, h, bias, bias_f32, dh, partial, db, db_f32, R, C,
                    stream);
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers; what the caller has checked is in launchers.h
// ---------------------------------------------------------------------------

extern "C" {

void bagua_bias_gelu_fwd_launch(int dtype, int tanh_form, const void* h,
                                const void* bias, int bias_f32, void* a,
                                size_t R, int C, hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, fwd_t, tanh_form, h, bias, bias_f32, a, R,
                 (size_t)C, stream);
}

size_t bagua_bias_gelu_partial_rows(size_t R, int C) {
  return row_blocks(R, (size_t)C, true);
}

void bagua_bias_gelu_bwd_launch(int dtype, int tanh_form, const void* dy,
                                const void* h, const void* bias, int bias_f32,
                                void* dh, float* partial, void* db,
                                int db_f32, size_t R, int C,
                                hipStream_t stream) {
  if (!bias || !db) partial = nullptr;
  DISPATCH_DTYPE(dtype, bf16_t, bwd_t, tanh_form, dy, h, bias, bias_f32, dh,
                 partial, db, db_f32, R, (size_t)C, stream);
}

}  // extern "C"
