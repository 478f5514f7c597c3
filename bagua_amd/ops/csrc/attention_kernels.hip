// CDNA4 (gfx950) self-attention over a packed qkv with a length per sequence,
// forward and backward, on the 32x32x16 MFMA instructions (bf16 and f16,
// head_dim 64).
//
//   qkv  (B, S, 3H), last dimension (3, heads, 64), as a Linear leaves it
//   out  (B, S, H)            lse  (B, heads, S) f32, natural logarithm
//   dqkv (B, S, 3H)
//
// For sequence b of length L = clamp(seq_lens[b], 0, S) and each head:
//   s = (q / 8) K[:L]^T     p = softmax(s)      out = p V[:L]      rows < L
//   dv = p^T dout   dp = dout V^T   ds = p * (dp - delta)   delta = rowsum(dout * out)
//   dq = ds K / 8   dk = ds^T (q / 8)
// Rows >= L of out and dqkv are written as zeros; rows >= L of qkv, dout and
// out are never loaded (a zero stands in for them), so nothing stored there,
// NaN included, reaches a result.
//
// How the matrices meet the MFMA. D = A B with A 32 x 16 and B 16 x 32: lane
// l holds 8 consecutive k of row (l % 32) of A and of column (l % 32) of B,
// the k of half (l / 32); D has column (l % 32) in the lane and rows
// 8 * (r / 4) + 4 * (l / 32) + r % 4 in its 16 registers r. Every product
// here is set up transposed, so that the matrix that stays for the whole
// kernel is the B operand, loaded once from global memory in 16-byte pieces
// into registers, and so that a D is the B of the next product as it lies:
// registers 8t .. 8t + 7 of a lane are the 8 values of k-step t (the k of a
// lane are then 4 + 4 rows, 8 apart; the A operand is read to match).
//
//   att_fwd    one block of 4 waves per (tile of 128 queries, head, sequence),
//              a wave has 32 queries. Q / 8 (exact) stays in registers as B.
//              Per tile of 64 keys: K goes to LDS as it lies, V transposed
//              (d-major), with 16-byte global loads; S^T = K Q^T (8 MFMA);
//              the lane's column is one query, so the running maximum and
//              sum are per lane, with one exchange between the halves; exp2
//              in f32; P is rounded only as the operand of
//              O^T += V^T P^T (8 MFMA). The loop ends at ceil(L / 64); a
//              block whose queries start at or behind L writes zeros.
//   att_delta  delta = rowsum(dout * out) per (row, head), 8 lanes a row.
//   att_dq     the same blocks as forward. Q / 8 and dout^T in registers;
//              K, V as they lie and K transposed in LDS; per 32 keys
//              S^T = K Q^T, dP^T = V dout^T, dS^T in registers,
//              dQ^T += K^T dS^T.
//   att_dkdv   one block per (tile of 128 keys, head, sequence), a wave has
//              32 keys, K and V in registers as B. Per tile of 64 queries:
//              Q / 8 and dout in LDS both as they lie and transposed, lse
//              and delta beside them; per 32 queries S = Q K^T,
//              dP = dout V^T, then dV^T += dout^T P and dK^T += (Q / 8)^T dS.
//
// Every result tile leaves through LDS, turned back to rows, in 16-byte
// stores at its place in out or in its third of dqkv. No atomics: a result
// element has one block and a fixed order of sums.

#include <hip/hip_runtime.h>  // by name in every .hip file: see device_util.h

#include "device_util.h"
#include "launchers.h"

#define ATT_BM BAGUA_ATT_BLOCK_M
#define ATT_BN BAGUA_ATT_BLOCK_N
#define ATT_THREADS 256
// LDS row strides in elements: a tile as it lies (16-byte reads of 8 d) and
// transposed (8-byte reads of 4 rows)
#define ATT_KS 72
#define ATT_TS 68
#define ATT_ROWS_EL (ATT_BN * ATT_KS)
#define ATT_TR_EL (ATT_BN * ATT_TS)
// a result tile on its way out: 32 rows a wave
#define ATT_OUT_EL (4 * 32 * ATT_KS)

#define ATT_KERNEL \
  __global__ void __launch_bounds__(ATT_THREADS) NO_PACKED_F32

static_assert(ATT_BM == 128 && ATT_BN == 64 && BAGUA_ATT_HEAD_DIM == 64,
              "the kernels are written for these tiles");

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float kLog2e = 1.4426950408889634f;

// an element as its 16 bits
template <typename T> struct El;
template <> struct El<bf16_t> {
  static __device__ __forceinline__ float to(uint32_t b) {
    return bf16_to_f((uint16_t)b);
  }
  static __device__ __forceinline__ uint32_t from(float f) {
    return f_to_bf16(f);
  }
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(
        __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
        0);
#else
    return c;
#endif
  }
};
template <> struct El<__half> {
  static __device__ __forceinline__ float to(uint32_t b) {
    return __half2float(__ushort_as_half((unsigned short)b));
  }
  static __device__ __forceinline__ uint32_t from(float f) {
    return __half_as_ushort(__float2half(f));
  }
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(
        __builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
        0);
#else
    return c;
#endif
  }
};

template <typename T>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return El<T>::from(lo) | (El<T>::from(hi) << 16);
}

// 8 elements times 1/8: exact, a power of two
template <typename T>
__device__ __forceinline__ u32x4 eighth(u32x4 v) {
  u32x4 o;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    o[w] = pack2<T>(El<T>::to(v[w] & 0xFFFFu) * 0.125f,
                    El<T>::to(v[w] >> 16) * 0.125f);
  return o;
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

__device__ __forceinline__ int seq_len(const int* lens, int b, int S) {
  if (!lens) return S;
  const int l = lens[b];
  return l < 0 ? 0 : (l > S ? S : l);
}

// 8 elements of row `row`, zero at or behind `limit`
__device__ __forceinline__ u32x4 load_row8(const uint16_t* base, size_t stride,
                                           int row, int limit, int d) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (row < limit)
    v = *reinterpret_cast<const u32x4*>(base + (size_t)row * stride + d);
  return v;
}

// The registers of a lane that stay as B: 8 d of k-step t of its row.
template <typename T, bool SCALE>
__device__ __forceinline__ void load_b(u32x4 (&f)[4], const uint16_t* base,
                                       size_t stride, int row, int limit,
                                       int half) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f[t] = load_row8(base, stride, row, limit, 16 * t + 8 * half);
    if (SCALE) f[t] = eighth<T>(f[t]);
  }
}

// Rows row0 .. row0 + 63 of a head's 64 columns into LDS: as they lie
// (`rows`, stride ATT_KS) and / or transposed (`tr`, stride ATT_TS); either
// may be null. A thread has one 16-byte chunk of two neighbouring rows and
// writes the pair's 8 columns as 8 words of the transposed tile.
template <typename T, bool SCALE>
__device__ __forceinline__ void stage(uint16_t* rows, uint16_t* tr,
                                      const uint16_t* base, size_t stride,
                                      int row0, int limit) {
  const int c = threadIdx.x & 7, pair = threadIdx.x >> 3;  // 32 pairs
  u32x4 v0 = load_row8(base, stride, row0 + 2 * pair, limit, 8 * c);
  u32x4 v1 = load_row8(base, stride, row0 + 2 * pair + 1, limit, 8 * c);
  if (SCALE) {
    v0 = eighth<T>(v0);
    v1 = eighth<T>(v1);
  }
  if (rows) {
    *reinterpret_cast<u32x4*>(rows + (2 * pair) * ATT_KS + 8 * c) = v0;
    *reinterpret_cast<u32x4*>(rows + (2 * pair + 1) * ATT_KS + 8 * c) = v1;
  }
  if (tr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t a = (e & 1) ? (v0[e >> 1] >> 16) : (v0[e >> 1] & 0xFFFFu);
      const uint32_t b = (e & 1) ? (v1[e >> 1] >> 16) : (v1[e >> 1] & 0xFFFFu);
      *reinterpret_cast<uint32_t*>(tr + (8 * c + e) * ATT_TS + 2 * pair) =
          a | (b << 16);
    }
  }
}

// A of a product over the rows of a tile that lies as rows: row `row`, 8 d
__device__ __forceinline__ u32x4 a_rows(const uint16_t* rows, int row, int t,
                                        int half) {
  return *reinterpret_cast<const u32x4*>(rows + row * ATT_KS + 16 * t +
                                         8 * half);
}

// A of a product over a transposed tile: d `d`, the 4 + 4 rows of k-step t2
// of block `blk` (32 rows) that registers 8 * t2 .. 8 * t2 + 7 of a D hold
__device__ __forceinline__ u32x4 a_tr(const uint16_t* tr, int d, int blk,
                                      int t2, int half) {
  const uint16_t* p = tr + d * ATT_TS + 32 * blk + 16 * t2 + 4 * half;
  const u32x2 lo = *reinterpret_cast<const u32x2*>(p);
  const u32x2 hi = *reinterpret_cast<const u32x2*>(p + 8);
  u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return v;
}

// registers 8 * t2 .. 8 * t2 + 7 of 16 rounded values, as B
__device__ __forceinline__ u32x4 b_regs(const uint32_t (&w)[8], int t2) {
  u32x4 v = {w[4 * t2], w[4 * t2 + 1], w[4 * t2 + 2], w[4 * t2 + 3]};
  return v;
}

// zeros in rows row0 .. row0 + 127 (below S) of a head's 64 columns
__device__ __forceinline__ void zero_rows(uint16_t* base, size_t stride,
                                          int row0, int S) {
  const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = threadIdx.x + ATT_THREADS * i;
    const int row = row0 + (idx >> 3);
    if (row < S)
      *reinterpret_cast<u32x4*>(base + (size_t)row * stride + 8 * (idx & 7)) =
          z;
  }
}

// A wave's D^T (its lane's column is row row0 + 32 * wave + col of the
// result, the registers are the 64 d), times `mul`, through LDS to global
// rows; rows at or behind L get zeros, rows at or behind S are not there.
// Every thread of the block calls it.
template <typename T>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[2], float mul,
                                           uint16_t* smem, uint16_t* base,
                                           size_t stride, int row0, int L,
                                           int S) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 31, half = lane >> 5;
  uint16_t* os = smem + wave * 32 * ATT_KS;
  __syncthreads();  // whatever lay in smem has been read
#pragma unroll
  for (int db = 0; db < 2; ++db) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32x2 w = {pack2<T>(acc[db][4 * g] * mul, acc[db][4 * g + 1] * mul),
                 pack2<T>(acc[db][4 * g + 2] * mul, acc[db][4 * g + 3] * mul)};
      *reinterpret_cast<u32x2*>(os + col * ATT_KS + 32 * db + 8 * g +
                                4 * half) = w;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = lane + 64 * i;
    const int r = idx >> 3, c = idx & 7;
    const int row = row0 + 32 * wave + r;
    if (row < S) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < L) v = *reinterpret_cast<const u32x4*>(os + r * ATT_KS + 8 * c);
      *reinterpret_cast<u32x4*>(base + (size_t)row * stride + 8 * c) = v;
    }
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

template <typename T>
ATT_KERNEL att_fwd_kernel(const uint16_t* __restrict__ qkv,
                          const int* __restrict__ lens,
                          uint16_t* __restrict__ out, float* __restrict__ lse,
                          int S, int heads) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[ATT_OUT_EL];
  static_assert(ATT_ROWS_EL + ATT_TR_EL <= ATT_OUT_EL, "K and V^T fit");
  uint16_t* ks = smem;
  uint16_t* vt = smem + ATT_ROWS_EL;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 31, half = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const size_t H = (size_t)heads * 64, rs = 3 * H;
  const int L = seq_len(lens, b, S);
  const int m0 = blockIdx.x * ATT_BM;

  const uint16_t* qb = qkv + (size_t)b * S * rs + (size_t)head * 64;
  const uint16_t* kb = qb + H;
  const uint16_t* vb = qb + 2 * H;
  uint16_t* ob = out + (size_t)b * S * H + (size_t)head * 64;
  float* lb = lse + ((size_t)b * heads + head) * S;
  const int q = m0 + 32 * wave + col;  // the lane's query

  if (m0 >= L) {  // the whole block
    zero_rows(ob, H, m0, S);
    if (half == 0 && q < S) lb[q] = 0.f;
    return;
  }

  u32x4 qf[4];
  load_b<T, true>(qf, qb, rs, q, L, half);

  f32x16 acc[2] = {zero16(), zero16()};
  float m = -INFINITY, lsum = 0.f;  // lsum: this half's keys only

  const int ntiles = (L + ATT_BN - 1) / ATT_BN;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int n0 = kt * ATT_BN;
    __syncthreads();  // the tile before has been read
    stage<T, false>(ks, nullptr, kb, rs, n0, L);
    stage<T, false>(nullptr, vt, vb, rs, n0, L);
    __syncthreads();

    f32x16 st[2] = {zero16(), zero16()};
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        st[blk] = El<T>::mfma(a_rows(ks, 32 * blk + col, t, half), qf[t],
                              st[blk]);

    // keys at or behind L drop out; the tile has a key in front of L
    float mx = -INFINITY;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = n0 + 32 * blk + 8 * (r >> 2) + 4 * half + (r & 3);
        const float v = key < L ? st[blk][r] : -INFINITY;
        st[blk][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float mls = m_new * kLog2e;
    const float alpha = __builtin_amdgcn_exp2f(m * kLog2e - mls);
    m = m_new;
    lsum *= alpha;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[db][r] *= alpha;

#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      uint32_t pw[8];
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float p0 = __builtin_amdgcn_exp2f(st[blk][r] * kLog2e - mls);
        const float p1 = __builtin_amdgcn_exp2f(st[blk][r + 1] * kLog2e - mls);
        lsum += p0;
        lsum += p1;
        pw[r >> 1] = pack2<T>(p0, p1);
      }
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const u32x4 pb = b_regs(pw, t2);
#pragma unroll
        for (int db = 0; db < 2; ++db)
          acc[db] = El<T>::mfma(a_tr(vt, 32 * db + col, blk, t2, half), pb,
                                acc[db]);
      }
    }
  }

  const float l = lsum + __shfl_xor(lsum, 32);
  if (half == 0 && q < S) lb[q] = q < L ? m + __logf(l) : 0.f;
  store_tile<T>(acc, 1.f / l, smem, ob, H, m0, L, S);
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// 8 lanes a (row, head): thread g has elements 8g .. 8g + 7 of (B, S, H)
template <typename T>
ATT_KERNEL att_delta_kernel(const uint16_t* __restrict__ dout,
                            const uint16_t* __restrict__ out,
                            const int* __restrict__ lens,
                            float* __restrict__ delta, int B, int S,
                            int heads) {
  const size_t g = (size_t)blockIdx.x * ATT_THREADS + threadIdx.x;
  const size_t total = (size_t)B * S * heads * 8;  // a multiple of 8
  const bool there = g < total;
  const size_t rh = g >> 3;
  const int head = (int)(rh % heads);
  const size_t row = rh / heads;
  const int b = there ? (int)(row / S) : 0, q = (int)(row % S);
  const bool live = there && q < seq_len(lens, b, S);
  float sum = 0.f;
  if (live) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(dout + g * 8);
    const u32x4 o = *reinterpret_cast<const u32x4*>(out + g * 8);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      sum += El<T>::to(a[w] & 0xFFFFu) * El<T>::to(o[w] & 0xFFFFu);
      sum += El<T>::to(a[w] >> 16) * El<T>::to(o[w] >> 16);
    }
  }
  sum += __shfl_xor(sum, 1);
  sum += __shfl_xor(sum, 2);
  sum += __shfl_xor(sum, 4);
  if (there && (g & 7) == 0)
    delta[((size_t)b * heads + head) * S + q] = live ? sum : 0.f;
}

template <typename T>
ATT_KERNEL att_dq_kernel(const uint16_t* __restrict__ dout,
                         const uint16_t* __restrict__ qkv,
                         const float* __restrict__ lse,
                         const float* __restrict__ delta,
                         const int* __restrict__ lens,
                         uint16_t* __restrict__ dqkv, int S, int heads) {
  __shared__ __attribute__((aligned(16)))
  uint16_t smem[2 * ATT_ROWS_EL + ATT_TR_EL];
  static_assert(ATT_OUT_EL <= 2 * ATT_ROWS_EL + ATT_TR_EL, "dQ fits");
  uint16_t* ks = smem;
  uint16_t* vs = smem + ATT_ROWS_EL;
  uint16_t* kt_s = smem + 2 * ATT_ROWS_EL;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 31, half = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const size_t H = (size_t)heads * 64, rs = 3 * H;
  const int L = seq_len(lens, b, S);
  const int m0 = blockIdx.x * ATT_BM;

  const uint16_t* qb = qkv + (size_t)b * S * rs + (size_t)head * 64;
  const uint16_t* kb = qb + H;
  const uint16_t* vb = qb + 2 * H;
  const uint16_t* gb = dout + (size_t)b * S * H + (size_t)head * 64;
  uint16_t* dqb = dqkv + (size_t)b * S * rs + (size_t)head * 64;
  const size_t stat = ((size_t)b * heads + head) * S;
  const int q = m0 + 32 * wave + col;

  if (m0 >= L) {
    zero_rows(dqb, rs, m0, S);
    return;
  }

  u32x4 qf[4], gf[4];
  load_b<T, true>(qf, qb, rs, q, L, half);
  load_b<T, false>(gf, gb, H, q, L, half);
  const float lse_l2 = (q < L ? lse[stat + q] : 0.f) * kLog2e;
  const float dl = q < L ? delta[stat + q] : 0.f;

  f32x16 acc[2] = {zero16(), zero16()};
  const int ntiles = (L + ATT_BN - 1) / ATT_BN;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int n0 = kt * ATT_BN;
    __syncthreads();
    stage<T, false>(ks, kt_s, kb, rs, n0, L);
    stage<T, false>(vs, nullptr, vb, rs, n0, L);
    __syncthreads();

#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      f32x16 st = zero16(), dp = zero16();
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        st = El<T>::mfma(a_rows(ks, 32 * blk + col, t, half), qf[t], st);
        dp = El<T>::mfma(a_rows(vs, 32 * blk + col, t, half), gf[t], dp);
      }
      uint32_t dw[8];
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        float ds[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int rr = r + j;
          const int key = n0 + 32 * blk + 8 * (rr >> 2) + 4 * half + (rr & 3);
          const float p =
              key < L ? __builtin_amdgcn_exp2f(st[rr] * kLog2e - lse_l2) : 0.f;
          ds[j] = p * (dp[rr] - dl);
        }
        dw[r >> 1] = pack2<T>(ds[0], ds[1]);
      }
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const u32x4 db_ = b_regs(dw, t2);
#pragma unroll
        for (int db = 0; db < 2; ++db)
          acc[db] = El<T>::mfma(a_tr(kt_s, 32 * db + col, blk, t2, half), db_,
                                acc[db]);
      }
    }
  }
  store_tile<T>(acc, 0.125f, smem, dqb, rs, m0, L, S);
}

template <typename T>
ATT_KERNEL att_dkdv_kernel(const uint16_t* __restrict__ dout,
                           const uint16_t* __restrict__ qkv,
                           const float* __restrict__ lse,
                           const float* __restrict__ delta,
                           const int* __restrict__ lens,
                           uint16_t* __restrict__ dqkv, int S, int heads) {
  __shared__ __attribute__((aligned(16)))
  uint16_t smem[2 * ATT_ROWS_EL + 2 * ATT_TR_EL];
  __shared__ float lse_s[ATT_BN], delta_s[ATT_BN];
  static_assert(ATT_OUT_EL <= 2 * ATT_ROWS_EL + 2 * ATT_TR_EL, "dK fits");
  uint16_t* qs = smem;
  uint16_t* gs = smem + ATT_ROWS_EL;
  uint16_t* qt = smem + 2 * ATT_ROWS_EL;
  uint16_t* gt = qt + ATT_TR_EL;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 31, half = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const size_t H = (size_t)heads * 64, rs = 3 * H;
  const int L = seq_len(lens, b, S);
  const int n0 = blockIdx.x * ATT_BM;  // 128 keys a block

  const uint16_t* qb = qkv + (size_t)b * S * rs + (size_t)head * 64;
  const uint16_t* kb = qb + H;
  const uint16_t* vb = qb + 2 * H;
  const uint16_t* gb = dout + (size_t)b * S * H + (size_t)head * 64;
  uint16_t* dkb = dqkv + (size_t)b * S * rs + H + (size_t)head * 64;
  uint16_t* dvb = dkb + H;
  const size_t stat = ((size_t)b * heads + head) * S;
  const int key = n0 + 32 * wave + col;

  if (n0 >= L) {
    zero_rows(dkb, rs, n0, S);
    zero_rows(dvb, rs, n0, S);
    return;
  }

  u32x4 kf[4], vf[4];
  load_b<T, false>(kf, kb, rs, key, L, half);
  load_b<T, false>(vf, vb, rs, key, L, half);

  f32x16 dk[2] = {zero16(), zero16()}, dv[2] = {zero16(), zero16()};
  const int ntiles = (L + ATT_BN - 1) / ATT_BN;
  for (int it = 0; it < ntiles; ++it) {
    const int m0 = it * ATT_BN;
    __syncthreads();
    stage<T, true>(qs, qt, qb, rs, m0, L);
    stage<T, false>(gs, gt, gb, H, m0, L);
    if (threadIdx.x < ATT_BN) {
      const int qq = m0 + threadIdx.x;
      lse_s[threadIdx.x] = (qq < L ? lse[stat + qq] : 0.f) * kLog2e;
      delta_s[threadIdx.x] = qq < L ? delta[stat + qq] : 0.f;
    }
    __syncthreads();

#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s = El<T>::mfma(a_rows(qs, 32 * blk + col, t, half), kf[t], s);
        dp = El<T>::mfma(a_rows(gs, 32 * blk + col, t, half), vf[t], dp);
      }
      uint32_t pw[8], dw[8];
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        float p[2], ds[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int rr = r + j;
          const int qi = 32 * blk + 8 * (rr >> 2) + 4 * half + (rr & 3);
          p[j] = m0 + qi < L
                     ? __builtin_amdgcn_exp2f(s[rr] * kLog2e - lse_s[qi])
                     : 0.f;
          ds[j] = p[j] * (dp[rr] - delta_s[qi]);
        }
        pw[r >> 1] = pack2<T>(p[0], p[1]);
        dw[r >> 1] = pack2<T>(ds[0], ds[1]);
      }
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const u32x4 pb = b_regs(pw, t2), db_ = b_regs(dw, t2);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          dv[db] = El<T>::mfma(a_tr(gt, 32 * db + col, blk, t2, half), pb,
                               dv[db]);
          dk[db] = El<T>::mfma(a_tr(qt, 32 * db + col, blk, t2, half), db_,
                               dk[db]);
        }
      }
    }
  }
  store_tile<T>(dk, 1.f, smem, dkb, rs, n0, L, S);  // Q came in as Q / 8
  store_tile<T>(dv, 1.f, smem, dvb, rs, n0, L, S);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

inline dim3 tile_grid(int B, int S, int heads) {
  return dim3((unsigned)((S + ATT_BM - 1) / ATT_BM), (unsigned)heads,
              (unsigned)B);
}

template <typename T>
void fwd_t(const void* qkv, const int* lens, void* out, float* lse, int B,
           int S, int heads, hipStream_t stream) {
  hipLaunchKernelGGL((att_fwd_kernel<T>), tile_grid(B, S, heads),
                     dim3(ATT_THREADS), 0, stream, (const uint16_t*)qkv, lens,
                     (uint16_t*)out, lse, S, heads);
}

template <typename T>
void bwd_t(const void* dout, const void* qkv, const void* out,
           const float* lse, const int* lens, float* delta, void* dqkv, int B,
           int S, int heads, hipStream_t stream) {
  const size_t chunks = (size_t)B * S * heads * 8;
  hipLaunchKernelGGL((att_delta_kernel<T>),
                     dim3((unsigned)((chunks + ATT_THREADS - 1) / ATT_THREADS)),
                     dim3(ATT_THREADS), 0, stream, (const uint16_t*)dout,
                     (const uint16_t*)out, lens, delta, B, S, heads);
  hipLaunchKernelGGL((att_dkdv_kernel<T>), tile_grid(B, S, heads),
                     dim3(ATT_THREADS), 0, stream, (const uint16_t*)dout,
                     (const uint16_t*)qkv, lse, (const float*)delta, lens,
                     (uint16_t*)dqkv, S, heads);
  hipLaunchKernelGGL((att_dq_kernel<T>), tile_grid(B, S, heads),
                     dim3(ATT_THREADS), 0, stream, (const uint16_t*)dout,
                     (const uint16_t*)qkv, lse, (const float*)delta, lens,
                     (uint16_t*)dqkv, S, heads);
}

// f32 has no MFMA path here
template <>
void fwd_t<float>(const void*, const int*, void*, float*, int, int, int,
                  hipStream_t) {
  throw std::invalid_argument("attention kernels take bf16 and f16");
}
template <>
void bwd_t<float>(const void*, const void*, const void*, const float*,
                  const int*, float*, void*, int, int, int, hipStream_t) {
  throw std::invalid_argument("attention kernels take bf16 and f16");
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers; what the caller has checked is in launchers.h
// ---------------------------------------------------------------------------

extern "C" {

void bagua_attention_fwd_launch(int dtype, const void* qkv,
                                const int* seq_lens, void* out, float* lse,
                                int B, int S, int heads, hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, fwd_t, qkv, seq_lens, out, lse, B, S, heads,
                 stream);
}

void bagua_attention_bwd_launch(int dtype, const void* dout, const void* qkv,
                                const void* out, const float* lse,
                                const int* seq_lens, float* delta, void* dqkv,
                                int B, int S, int heads, hipStream_t stream) {
  DISPATCH_DTYPE(dtype, bf16_t, bwd_t, dout, qkv, out, lse, seq_lens, delta,
                 dqkv, B, S, heads, stream);
}

}  // extern "C"
