// CDNA4 (gfx950) kernels for a transformer sub-layer's tail, forward and
// backward, over rows [R, H]:
//
//   s = x + keep * (h + bias) / (1 - p)         keep ~ Bernoulli(1 - p)
//   y = (s - mean(s)) * rstd(s) * gamma + beta
//
// x is the residual stream, h the branch (a Linear's output without its
// bias) and bias that Linear's bias. The torch chain is a dropout, an add
// and a LayerNorm kernel each way plus a row-sum for the bias gradient;
// here the forward is one kernel (read x and h, write y and s), the
// backward one kernel (read dy and s, write dx and dh) and a small second
// stage for the column sums. h may have two bytes per element under an f32
// x, which is what autocast hands over.
//
//   ln_fwd           a wave owns a row at a time. The row is cut into chunks
//                    of 8 elements (16 bytes of a 2-byte type, 32 of f32);
//                    chunk j belongs to lane j % 64 in iteration j / 64, and
//                    the lane keeps its chunks of s in registers as f32 for
//                    the whole row: nothing is read twice and the row needs
//                    no LDS. Mean by a wave reduction, then the variance as
//                    the mean of squared deviations from it, over the
//                    registers. Also stores s (rounded), mean and rstd, and
//                    with dropout a keep byte per chunk.
//   ln_bwd           the same shape. xhat = (s - mean) * rstd,
//                    dxhat = dy * gamma, two row means by wave reduction,
//                    ds = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat *
//                    xhat)), dh = ds * keep / (1 - p). A lane owns the same
//                    columns in every row it visits, so the column sums
//                    (dgamma += dy * xhat, dbeta += dy, dbias += dh) grow in
//                    its registers; at the end the block's waves are added
//                    through LDS in a fixed order into the block's row of an
//                    f32 buffer [blocks, 3H].
//   ln_bwd_finalize  adds those rows in a fixed order and writes the three
//                    gradients in their parameters' dtypes.
//
// Blocks are LN_WAVES waves and grid-stride over rows under a capped grid.
// All arithmetic is f32 with one rounding per stored value (bf16 as torch
// rounds). No atomics: every sum has a fixed order, so results are the same
// bits from run to run.
//
// Dropout bits come from Philox4x32-10, written out below, keyed by a
// 64-bit seed that the kernel reads from device memory (nothing of it is
// known to the host, so a captured graph replays with fresh seeds). The
// counter is the element's row-major index: one call with counter e / 4
// gives the 32-bit words of elements e .. e + 3. The mask is therefore a
// function of (seed, element index, p) alone, whatever the grid. Backward
// reads the stored bytes and never regenerates.

#include <hip/hip_runtime.h>  // by name in every .hip file: see device_util.h
#include <cmath>

#include "device_util.h"  // to_f / from_f (bf16 is bf16_t), Vec16
#include "launchers.h"

#define LN_BLOCK (64 * BAGUA_LN_WAVES)
// blocks of the backward kernel, rows of its partial buffer
#define LN_BWD_MAX_GRID 512
// finalize: 16 columns x 16 slices of the partial rows per block
#define LN_FIN_COLS 16
#define LN_FIN_SL (LN_BLOCK / LN_FIN_COLS)

#define LN_KERNEL \
  __global__ void __launch_bounds__(LN_BLOCK) NO_PACKED_F32

namespace {

// A per-column vector is f32 or T, told at run time; element access, as it
// may be a view into a flat parameter buffer and need not be aligned.
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

// the 8 columns from `col` on of a per-column vector, `fill` where it is null
template <typename T>
__device__ __forceinline__ void load_cols(const void* p, int is_f32, int col,
                                          float fill, float (&f)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k)
    f[k] = p ? ld_param<T>(p, is_f32, col + k) : fill;
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

// Sum over the wave; every lane gets the same bits (a butterfly of
// commutative additions).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Philox4x32-10 (Salmon et al., SC'11) of the counter (c0, 0, 0, 0) under
// the key (k0, k1).
struct Philox4 {
  uint32_t v[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t k0,
                                                 uint32_t k1) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 r;
  r.v[0] = c0;
  r.v[1] = c1;
  r.v[2] = c2;
  r.v[3] = c3;
  return r;
}

// keep bits of the chunk whose first element has row-major index e (a
// multiple of 8): bit k set where element e + k stays
__device__ __forceinline__ unsigned keep_bits(uint32_t e, uint32_t k0,
                                              uint32_t k1,
                                              uint32_t drop_threshold) {
  unsigned bits = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const Philox4 r = philox4x32_10((e >> 2) + q, k0, k1);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      bits |= (unsigned)(r.v[k] >= drop_threshold) << (4 * q + k);
  }
  return bits;
}

struct FwdArgs {
  const void* x;
  const void* h;      // null: plain LayerNorm of x
  const void* bias;   // of the branch; null or per column
  const void* gamma;  // null or per column
  const void* beta;
  int bias_f32, gamma_f32, beta_f32;
  const int64_t* seed;  // device memory; read only with mask
  uint32_t drop_threshold;
  float scale;  // 1 / (1 - p), 1 without dropout
  void* y;
  void* s;  // null: not stored
  float* mean;
  float* rstd;
  uint8_t* mask;  // null: no dropout
  float eps;
  int R, H;
};

// ITERS: chunks of a row that a lane holds, ceil(H / 8 / 64). Up to two,
// the lane also keeps its columns of bias, gamma and beta in registers for
// all its rows; beyond, it reads them again per row (from cache) to stay
// within its registers.
template <typename Tx, typename Th, int ITERS>
LN_KERNEL ln_fwd_kernel(FwdArgs a) {
  constexpr bool KEEP = ITERS <= 2;
  constexpr int KI = KEEP ? ITERS : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = a.H >> 3;
  const float inv_h = 1.f / (float)a.H;
  const Tx* x = static_cast<const Tx*>(a.x);
  const Th* h = static_cast<const Th*>(a.h);
  Tx* y = static_cast<Tx*>(a.y);
  Tx* s_out = static_cast<Tx*>(a.s);

  float cb[KI][8], cg[KI][8], ce[KI][8];
  if constexpr (KEEP) {
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int j = lane + 64 * i;
      if (j < nch) {
        load_cols<Th>(a.bias, a.bias_f32, j * 8, 0.f, cb[i]);
        load_cols<Tx>(a.gamma, a.gamma_f32, j * 8, 1.f, cg[i]);
        load_cols<Tx>(a.beta, a.beta_f32, j * 8, 0.f, ce[i]);
      }
    }
  }
  uint32_t k0 = 0, k1 = 0;
  if (a.mask) {
    const uint32_t* sp = reinterpret_cast<const uint32_t*>(a.seed);
    k0 = sp[0];
    k1 = sp[1];
  }

  for (int r = blockIdx.x * BAGUA_LN_WAVES + wave; r < a.R;
       r += gridDim.x * BAGUA_LN_WAVES) {
    const size_t row = (size_t)r * a.H;
    float s[ITERS][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int j = lane + 64 * i;
      if (j < nch) {
        load8<Tx>(x + row + j * 8, s[i]);
        if (h) {
          float v[8];
          load8<Th>(h + row + j * 8, v);
          if constexpr (!KEEP)
            load_cols<Th>(a.bias, a.bias_f32, j * 8, 0.f, cb[0]);
          unsigned bits = 0xFFu;
          if (a.mask) {
            bits = keep_bits((uint32_t)(row + j * 8), k0, k1,
                             a.drop_threshold);
            a.mask[(size_t)r * nch + j] = (uint8_t)bits;
          }
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (bits >> k & 1u)
              s[i][k] += (v[k] + cb[KEEP ? i : 0][k]) * a.scale;
        }
        if (s_out) store8<Tx>(s_out + row + j * 8, s[i]);
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += s[i][k];
      }
    }
    const float mean = wave_sum(sum) * inv_h;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      if (lane + 64 * i < nch) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = s[i][k] - mean;
          sq += d * d;
        }
      }
    }
    const float rstd = 1.f / sqrtf(wave_sum(sq) * inv_h + a.eps);
    if (lane == 0) {
      a.mean[r] = mean;
      a.rstd[r] = rstd;
    }
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int j = lane + 64 * i;
      if (j < nch) {
        if constexpr (!KEEP) {
          load_cols<Tx>(a.gamma, a.gamma_f32, j * 8, 1.f, cg[0]);
          load_cols<Tx>(a.beta, a.beta_f32, j * 8, 0.f, ce[0]);
        }
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          o[k] = (s[i][k] - mean) * rstd * cg[KEEP ? i : 0][k] +
                 ce[KEEP ? i : 0][k];
        store8<Tx>(y + row + j * 8, o);
      }
    }
  }
}

struct BwdArgs {
  const void* dy;
  const void* s;
  const float* mean;
  const float* rstd;
  const void* gamma;  // null or per column
  int gamma_f32;
  const uint8_t* mask;  // null: no dropout
  float scale;
  int has_branch;
  void* dx;
  void* dh;        // null: not written
  float* partial;  // [gridDim.x, 3H]: dgamma, dbeta, dbias; null: no sums
  int want_gamma, want_beta, want_bias;
  int R, H;
};

// The waves' accumulators of one column sum, added in the order of the
// waves and stored to dst[0 .. H). Every thread of the block calls.
template <int ITERS>
__device__ __forceinline__ void block_sum_store(const float (&acc)[ITERS][8],
                                                float (*red)[512], int H,
                                                float* __restrict__ dst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wave][lane * 8 + k] = acc[i][k];
    __syncthreads();
    for (int idx = threadIdx.x; idx < 512; idx += LN_BLOCK) {
      const int col = i * 512 + idx;
      if (col < H) {
        float t = red[0][idx];
#pragma unroll
        for (int w = 1; w < BAGUA_LN_WAVES; ++w) t += red[w][idx];
        dst[col] = t;
      }
    }
  }
}

template <typename Tx, typename Th, int ITERS>
LN_KERNEL ln_bwd_kernel(BwdArgs a) {
  __shared__ float red[BAGUA_LN_WAVES][512];
  constexpr bool KEEP = ITERS <= 2;
  constexpr int KI = KEEP ? ITERS : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = a.H >> 3;
  const float inv_h = 1.f / (float)a.H;
  const Tx* dy = static_cast<const Tx*>(a.dy);
  const Tx* s = static_cast<const Tx*>(a.s);
  Tx* dx = static_cast<Tx*>(a.dx);
  Th* dh = static_cast<Th*>(a.dh);

  float cg[KI][8];
  if constexpr (KEEP) {
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int j = lane + 64 * i;
      if (j < nch) load_cols<Tx>(a.gamma, a.gamma_f32, j * 8, 1.f, cg[i]);
    }
  }
  float acc_g[ITERS][8], acc_b[ITERS][8], acc_h[ITERS][8];
#pragma unroll
  for (int i = 0; i < ITERS; ++i)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc_g[i][k] = acc_b[i][k] = acc_h[i][k] = 0.f;

  for (int r = blockIdx.x * BAGUA_LN_WAVES + wave; r < a.R;
       r += gridDim.x * BAGUA_LN_WAVES) {
    const size_t row = (size_t)r * a.H;
    const float mean = a.mean[r], rstd = a.rstd[r];
    float dxh[ITERS][8], xh[ITERS][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int j = lane + 64 * i;
      if (j < nch) {
        float d[8];
        load8<Tx>(dy + row + j * 8, d);
        load8<Tx>(s + row + j * 8, xh[i]);
        if constexpr (!KEEP)
          load_cols<Tx>(a.gamma, a.gamma_f32, j * 8, 1.f, cg[0]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          xh[i][k] = (xh[i][k] - mean) * rstd;
          acc_g[i][k] += d[k] * xh[i][k];
          acc_b[i][k] += d[k];
          dxh[i][k] = d[k] * cg[KEEP ? i : 0][k];
          s1 += dxh[i][k];
          s2 += dxh[i][k] * xh[i][k];
        }
      }
    }
    const float m1 = wave_sum(s1) * inv_h, m2 = wave_sum(s2) * inv_h;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
      const int j = lane + 64 * i;
      if (j < nch) {
        float g[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          g[k] = rstd * (dxh[i][k] - m1 - xh[i][k] * m2);
        store8<Tx>(dx + row + j * 8, g);
        if (a.has_branch) {
          if (a.mask) {
            const unsigned bits = a.mask[(size_t)r * nch + j];
#pragma unroll
            for (int k = 0; k < 8; ++k)
              g[k] = (bits >> k & 1u) ? g[k] * a.scale : 0.f;
          }
          if (dh) store8<Th>(dh + row + j * 8, g);
#pragma unroll
          for (int k = 0; k < 8; ++k) acc_h[i][k] += g[k];
        }
      }
    }
  }

  if (!a.partial) return;
  float* prow = a.partial + (size_t)blockIdx.x * 3 * a.H;
  if (a.want_gamma) block_sum_store<ITERS>(acc_g, red, a.H, prow);
  if (a.want_beta) block_sum_store<ITERS>(acc_b, red, a.H, prow + a.H);
  if (a.want_bias) block_sum_store<ITERS>(acc_h, red, a.H, prow + 2 * a.H);
}

// Column c of sum q (blockIdx.y: dgamma, dbeta, dbias) of the [nrows, 3H]
// partials, rows added in a fixed order: 16 slices per column keep a
// thread's chain of loads short, their results are added pairwise.
template <typename Tx, typename Th>
LN_KERNEL ln_bwd_finalize_kernel(const float* __restrict__ partial, int nrows,
                                 int H, void* dgamma, int dgamma_f32,
                                 void* dbeta, int dbeta_f32, void* dbias,
                                 int dbias_f32) {
  __shared__ float red[LN_FIN_SL][LN_FIN_COLS];
  const int q = blockIdx.y;
  void* out = q == 0 ? dgamma : q == 1 ? dbeta : dbias;
  if (!out) return;  // the whole block
  const int cl = threadIdx.x % LN_FIN_COLS, sl = threadIdx.x / LN_FIN_COLS;
  const int c = blockIdx.x * LN_FIN_COLS + cl;
  float t = 0.f;
  if (c < H) {
#pragma unroll 4
    for (int r = sl; r < nrows; r += LN_FIN_SL)
      t += partial[(size_t)r * 3 * H + (size_t)q * H + c];
  }
  red[sl][cl] = t;
  __syncthreads();
  for (int half = LN_FIN_SL / 2; half > 0; half /= 2) {
    if (sl < half) red[sl][cl] += red[sl + half][cl];
    __syncthreads();
  }
  if (sl == 0 && c < H) {
    if (q == 0)
      st_param<Tx>(out, dgamma_f32, c, red[0][cl]);
    else if (q == 1)
      st_param<Tx>(out, dbeta_f32, c, red[0][cl]);
    else
      st_param<Th>(out, dbias_f32, c, red[0][cl]);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

inline unsigned ln_grid(int R, unsigned cap) {
  unsigned blocks = ((unsigned)R + BAGUA_LN_WAVES - 1) / BAGUA_LN_WAVES;
  if (blocks > cap) blocks = cap;
  return blocks ? blocks : 1;
}

struct BwdOut {
  void* dgamma;
  void* dbeta;
  void* dbias;
  int dgamma_f32, dbeta_f32, dbias_f32;
};

template <typename Tx, typename Th, int ITERS>
void fwd_i(const FwdArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL((ln_fwd_kernel<Tx, Th, ITERS>),
                     dim3(ln_grid(a.R, BAGUA_LN_FWD_MAX_GRID)),
                     dim3(LN_BLOCK), 0, stream, a);
}

template <typename Tx, typename Th, int ITERS>
void bwd_i(const BwdArgs& a, const BwdOut& o, hipStream_t stream) {
  const unsigned blocks = ln_grid(a.R, LN_BWD_MAX_GRID);
  hipLaunchKernelGGL((ln_bwd_kernel<Tx, Th, ITERS>), dim3(blocks),
                     dim3(LN_BLOCK), 0, stream, a);
  if (!a.partial) return;
  hipLaunchKernelGGL((ln_bwd_finalize_kernel<Tx, Th>),
                     dim3((a.H + LN_FIN_COLS - 1) / LN_FIN_COLS, 3),
                     dim3(LN_BLOCK), 0, stream, a.partial, (int)blocks, a.H,
                     o.dgamma, o.dgamma_f32, o.dbeta, o.dbeta_f32, o.dbias,
                     o.dbias_f32);
}

// a lane's chunks: 1, 2, 4 or 8 for H up to 512, 1024, 2048, BAGUA_LN_HMAX
#define LN_DISPATCH_ITERS(H, fn, ...)                  \
  do {                                                 \
    const int chunks_ = (H) / 8;                       \
    if (chunks_ <= 64)                                 \
      fn<Tx, Th, 1>(__VA_ARGS__);                      \
    else if (chunks_ <= 128)                           \
      fn<Tx, Th, 2>(__VA_ARGS__);                      \
    else if (chunks_ <= 256)                           \
      fn<Tx, Th, 4>(__VA_ARGS__);                      \
    else                                               \
      fn<Tx, Th, 8>(__VA_ARGS__);                      \
  } while (0)

template <typename Tx, typename Th>
void fwd_h(const FwdArgs& a, hipStream_t stream) {
  LN_DISPATCH_ITERS(a.H, fwd_i, a, stream);
}
template <typename Tx, typename Th>
void bwd_h(const BwdArgs& a, const BwdOut& o, hipStream_t stream) {
  LN_DISPATCH_ITERS(a.H, bwd_i, a, o, stream);
}

// the branch has x's type, or two bytes per element under an f32 x
template <typename Tx>
void fwd_t(int x_dtype, int h_dtype, const FwdArgs& a, hipStream_t stream) {
  if (h_dtype == x_dtype) return fwd_h<Tx, Tx>(a, stream);
  if (x_dtype != BAGUA_F32)
    throw std::invalid_argument("a branch of another dtype needs an f32 x");
  if (h_dtype == BAGUA_F16) return fwd_h<float, __half>(a, stream);
  if (h_dtype == BAGUA_BF16) return fwd_h<float, bf16_t>(a, stream);
  throw std::invalid_argument("unknown kernel dtype code");
}
template <typename Tx>
void bwd_t(int x_dtype, int h_dtype, const BwdArgs& a, const BwdOut& o,
           hipStream_t stream) {
  if (h_dtype == x_dtype) return bwd_h<Tx, Tx>(a, o, stream);
  if (x_dtype != BAGUA_F32)
    throw std::invalid_argument("a branch of another dtype needs an f32 x");
  if (h_dtype == BAGUA_F16) return bwd_h<float, __half>(a, o, stream);
  if (h_dtype == BAGUA_BF16) return bwd_h<float, bf16_t>(a, o, stream);
  throw std::invalid_argument("unknown kernel dtype code");
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers; what the caller has checked is in launchers.h
// ---------------------------------------------------------------------------

extern "C" {

void bagua_ln_fwd_launch(int x_dtype, int h_dtype, const void* x,
                         const void* h, const void* bias, int bias_f32,
                         const void* gamma, int gamma_f32, const void* beta,
                         int beta_f32, const int64_t* seed,
                         uint32_t drop_threshold, float scale, void* y,
                         void* s, float* mean, float* rstd, uint8_t* mask,
                         float eps, size_t R, int H, hipStream_t stream) {
  FwdArgs a;
  a.x = x;
  a.h = h;
  a.bias = h ? bias : nullptr;
  a.gamma = gamma;
  a.beta = beta;
  a.bias_f32 = bias_f32;
  a.gamma_f32 = gamma_f32;
  a.beta_f32 = beta_f32;
  a.seed = seed;
  a.drop_threshold = drop_threshold;
  a.scale = (h && mask) ? scale : 1.f;
  a.y = y;
  a.s = s;
  a.mean = mean;
  a.rstd = rstd;
  a.mask = h ? mask : nullptr;
  a.eps = eps;
  a.R = (int)R;
  a.H = H;
  DISPATCH_DTYPE(x_dtype, bf16_t, fwd_t, x_dtype, h_dtype, a, stream);
}

size_t bagua_ln_partial_rows(size_t R) {
  return ln_grid((int)R, LN_BWD_MAX_GRID);
}

void bagua_ln_bwd_launch(int x_dtype, int h_dtype, const void* dy,
                         const void* s, const float* mean, const float* rstd,
                         const void* gamma, int gamma_f32,
                         const uint8_t* mask, float scale, int has_branch,
                         void* dx, void* dh, float* partial, void* dgamma,
                         int dgamma_f32, void* dbeta, int dbeta_f32,
                         void* dbias, int dbias_f32, size_t R, int H,
                         hipStream_t stream) {
  BwdOut o;
  o.dgamma = dgamma;
  o.dbeta = dbeta;
  o.dbias = has_branch ? dbias : nullptr;
  o.dgamma_f32 = dgamma_f32;
  o.dbeta_f32 = dbeta_f32;
  o.dbias_f32 = dbias_f32;
  BwdArgs a;
  a.dy = dy;
  a.s = s;
  a.mean = mean;
  a.rstd = rstd;
  a.gamma = gamma;
  a.gamma_f32 = gamma_f32;
  a.mask = has_branch ? mask : nullptr;
  a.scale = a.mask ? scale : 1.f;
  a.has_branch = has_branch;
  a.dx = dx;
  a.dh = has_branch ? dh : nullptr;
  a.want_gamma = o.dgamma != nullptr;
  a.want_beta = o.dbeta != nullptr;
  a.want_bias = o.dbias != nullptr;
  a.partial =
      (a.want_gamma || a.want_beta || a.want_bias) ? partial : nullptr;
  a.R = (int)R;
  a.H = H;
  DISPATCH_DTYPE(x_dtype, bf16_t, bwd_t, x_dtype, h_dtype, a, o, stream);
}

}  // extern "C"
