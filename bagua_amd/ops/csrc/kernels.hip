// CDNA4 (gfx950) kernel pack for bagua_amd.
//
// From-scratch MI355X implementations of the device math the reference
// framework shipped as CUDA (reference inventory:
// rust/bagua-core/bagua-core-internal/kernels/bagua_kernels.cu:196-501):
// elementwise bucket ops, chunked in-place reduce, MinMaxUInt8
// compress/decompress.
//
// Design (per the CDNA4 programming guide):
//  * 256-thread workgroups (4 waves of 64);
//  * every kernel is memory-bound -> 16-byte vectorized loads/stores per
//    lane (guide G13: scalar bf16/f16 loads are ~2-2.5x slower);
//  * grid capped at ~2048 workgroups with grid-stride loops (guide G11);
//  * min/max reductions: wave shuffle reduce over 64 lanes, then LDS
//    across the 4 waves, then one ordered-uint atomic per block
//    (guide: Reduction quick reference);
//  * float32 accumulation for f16/bf16 inputs.
//
// Compression wire format (matches bagua_amd/ops/quant.py, the numerics
// oracle): per chunk a 32-byte header whose first 8 bytes are (min,max)
// as float32 and whose bytes 8..31 are zero, then chunk uint8 payload
// bytes, then zero padding up to ceil32(chunk). quantize_kernel writes
// every byte of the chunk regions it is asked for.
//   scale = 255/(max-min+1e-7); upper = rint(max*scale);
//   lower = upper-255; q = clamp(min(rint(x*scale), upper) - lower, 0, 255).

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#define BLOCK 256
#define MAX_GRID 2048

// ---------------------------------------------------------------------------
// dtype helpers
// ---------------------------------------------------------------------------

template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<__half>(__half v) {
  return __half2float(v);
}
template <> __device__ __forceinline__ float to_f<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}

template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f<__half>(float v) {
  return __float2half(v);
}
template <> __device__ __forceinline__ __hip_bfloat16 from_f<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

// 16-byte per-lane vector of T. Access widths are now tuned PER KERNEL:
// elementwise uses 2x Vec16 (32 B), the compressor kernels use a fixed
// 16 u8 payload granule (16 B) with 16*sizeof(T)/16 Vec16 tensor-side
// vectors — the round-1 one-width-fits-all tradeoff is gone.
template <typename T> struct alignas(16) Vec16 {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

// ---------------------------------------------------------------------------
// elementwise ops: x = f(x, y)
// ---------------------------------------------------------------------------

enum EwOp { EW_AVERAGE = 0, EW_ADD = 1, EW_SUB = 2, EW_ADDMUL = 3, EW_DIV = 4 };

template <int OP>
__device__ __forceinline__ float ew_apply(float x, float y, float f) {
  if (OP == EW_AVERAGE) return (x + y) * 0.5f;
  if (OP == EW_ADD) return x + y;
  if (OP == EW_SUB) return x - y;
  if (OP == EW_ADDMUL) return x + y * f;
  return x * f;  // EW_DIV passes f = 1/divisor
}

template <typename T, int OP>
__global__ void ew_kernel(T* __restrict__ x, const T* __restrict__ y,
                          float f, size_t n) {
  // two 16-byte vectors per lane per iteration (32 B accesses): +9% on
  // the f32 read-modify-write pattern (round-1 measurement); unlike the
  // compressor kernels this path has no competing access width.
  constexpr int V = Vec16<T>::N;
  using VT = Vec16<T>;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv2 = n / (2 * V);

  VT* xv = reinterpret_cast<VT*>(x);
  const VT* yv = reinterpret_cast<const VT*>(y);
  for (size_t i = tid; i < nv2; i += stride) {
    VT a0 = xv[2 * i], a1 = xv[2 * i + 1];
    VT b0, b1;
    if (OP != EW_DIV) {
      b0 = yv[2 * i];
      b1 = yv[2 * i + 1];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float bx0 = (OP != EW_DIV) ? to_f(b0.v[k]) : 0.f;
      float bx1 = (OP != EW_DIV) ? to_f(b1.v[k]) : 0.f;
      a0.v[k] = from_f<T>(ew_apply<OP>(to_f(a0.v[k]), bx0, f));
      a1.v[k] = from_f<T>(ew_apply<OP>(to_f(a1.v[k]), bx1, f));
    }
    xv[2 * i] = a0;
    xv[2 * i + 1] = a1;
  }
  for (size_t i = nv2 * 2 * V + tid; i < n; i += stride) {
    float bx = (OP != EW_DIV) ? to_f(y[i]) : 0.f;
    x[i] = from_f<T>(ew_apply<OP>(to_f(x[i]), bx, f));
  }
}

// x += reduced / nranks - x_copy  (async model average,
// reference: bagua_kernels.cu:257-267)
template <typename T>
__global__ void async_avg_kernel(T* __restrict__ x,
                                 const T* __restrict__ reduced,
                                 const T* __restrict__ x_copy,
                                 float inv_n, size_t n) {
  constexpr int V = Vec16<T>::N;
  using VT = Vec16<T>;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = n / V;
  VT* xv = reinterpret_cast<VT*>(x);
  const VT* rv = reinterpret_cast<const VT*>(reduced);
  const VT* cv = reinterpret_cast<const VT*>(x_copy);
  for (size_t i = tid; i < nv; i += stride) {
    VT a = xv[i], r = rv[i], c = cv[i];
#pragma unroll
    for (int k = 0; k < V; ++k)
      a.v[k] = from_f<T>(to_f(a.v[k]) + to_f(r.v[k]) * inv_n - to_f(c.v[k]));
    xv[i] = a;
  }
  for (size_t i = nv * V + tid; i < n; i += stride)
    x[i] = from_f<T>(to_f(x[i]) + to_f(reduced[i]) * inv_n - to_f(x_copy[i]));
}

// ---------------------------------------------------------------------------
// chunked in-place reduce: x[target*chunk + i] = reduce_c x[c*chunk + i]
// (reference: bagua_kernels.cu:374-401) — vectorized over i, small loop
// over chunks accumulating in f32.
// ---------------------------------------------------------------------------

template <typename T>
__global__ void reduce_chunk_kernel(T* __restrict__ x, int num_chunks,
                                    int target_chunk, float post_scale,
                                    size_t chunk) {
  constexpr int V = Vec16<T>::N;
  using VT = Vec16<T>;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = chunk / V;
  VT* tv = reinterpret_cast<VT*>(x + (size_t)target_chunk * chunk);
  for (size_t i = tid; i < nv; i += stride) {
    float acc[Vec16<T>::N];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int c = 0; c < num_chunks; ++c) {
      const VT* cvp = reinterpret_cast<const VT*>(x + (size_t)c * chunk);
      VT b = cvp[i];
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += to_f(b.v[k]);
    }
    VT out;
#pragma unroll
    for (int k = 0; k < V; ++k) out.v[k] = from_f<T>(acc[k] * post_scale);
    tv[i] = out;
  }
  for (size_t i = nv * V + tid; i < chunk; i += stride) {
    float acc = 0.f;
    for (int c = 0; c < num_chunks; ++c) acc += to_f(x[(size_t)c * chunk + i]);
    x[(size_t)target_chunk * chunk + i] = from_f<T>(acc * post_scale);
  }
}

// ---------------------------------------------------------------------------
// MinMaxUInt8 compression
// ---------------------------------------------------------------------------

// monotonic float<->uint mapping so integer atomicMin/Max give float min/max
__device__ __forceinline__ uint32_t f32_to_ordered(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_f32(uint32_t u) {
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __uint_as_float(u);
}

#define MINMAX_MAX_BLOCKS 512

// stage 2: one block per chunk reduces the per-block partials (no
// atomics — 512 blocks contending on one address serialized ~100us)
__global__ void minmax_finalize_kernel(const uint32_t* __restrict__
                                       partials, int nblocks,
                                       int chunk_begin,
                                       uint32_t* __restrict__ scratch) {
  const int c = chunk_begin + blockIdx.x;
  const uint32_t* p = partials + (size_t)blockIdx.x * 2 * MINMAX_MAX_BLOCKS;
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x) {
    mn = min(mn, p[2 * i]);
    mx = max(mx, p[2 * i + 1]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = min(mn, (uint32_t)__shfl_down((int)mn, off, 64));
    mx = max(mx, (uint32_t)__shfl_down((int)mx, off, 64));
  }
  __shared__ uint32_t smn[BLOCK / 64], smx[BLOCK / 64];
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (lane == 0) {
    smn[wave] = mn;
    smx[wave] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) {
      mn = min(mn, smn[w]);
      mx = max(mx, smx[w]);
    }
    scratch[2 * c] = mn;
    scratch[2 * c + 1] = mx;
  }
}

// grid.y = chunk index (offset by chunk_begin); block-level min/max with
// wave shuffle + LDS across 4 waves, one atomic pair per block.
template <typename T>
__global__ void minmax_kernel(const T* __restrict__ x, size_t chunk,
                              int chunk_begin, uint32_t* partials) {
  constexpr int V = Vec16<T>::N;
  using VT = Vec16<T>;
  const int c = chunk_begin + blockIdx.y;
  const T* __restrict__ src = x + (size_t)c * chunk;

  // 4 independent accumulator pairs: a single (lmin,lmax) pair makes a
  // serial FP dependency chain per thread and the kernel goes
  // latency-bound (~1.2 TB/s measured); 4 chains restore ILP.
  float lmn[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  float lmx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = chunk / V;
  const VT* sv = reinterpret_cast<const VT*>(src);
  for (size_t i = tid; i < nv; i += stride) {
    VT a = sv[i];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float f = to_f(a.v[k]);
      lmn[k & 3] = fminf(lmn[k & 3], f);
      lmx[k & 3] = fmaxf(lmx[k & 3], f);
    }
  }
  for (size_t i = nv * V + tid; i < chunk; i += stride) {
    float f = to_f(src[i]);
    lmn[0] = fminf(lmn[0], f);
    lmx[0] = fmaxf(lmx[0], f);
  }
  float lmin = fminf(fminf(lmn[0], lmn[1]), fminf(lmn[2], lmn[3]));
  float lmax = fmaxf(fmaxf(lmx[0], lmx[1]), fmaxf(lmx[2], lmx[3]));

  // wave64 shuffle reduce
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lmin = fminf(lmin, __shfl_down(lmin, off, 64));
    lmax = fmaxf(lmax, __shfl_down(lmax, off, 64));
  }
  __shared__ float smin[BLOCK / 64], smax[BLOCK / 64];
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (lane == 0) {
    smin[wave] = lmin;
    smax[wave] = lmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) {
      lmin = fminf(lmin, smin[w]);
      lmax = fmaxf(lmax, smax[w]);
    }
    // per-block partial; chunk-row-local block index
    uint32_t* p = partials + (size_t)blockIdx.y * 2 * MINMAX_MAX_BLOCKS;
    p[2 * blockIdx.x] = f32_to_ordered(lmin);
    p[2 * blockIdx.x + 1] = f32_to_ordered(lmax);
  }
}

__device__ __forceinline__ void quant_params(float mn, float mx,
                                             float& scale, float& lower,
                                             float& upper) {
  scale = 255.0f / (mx - mn + 1e-7f);
  upper = rintf(mx * scale);
  lower = upper - 255.0f;
}

// level - lower leaves [0, 255] by a few units when |x|*scale > 2^24
// (constant chunks, |mean| >> range): the f32 roundings of level and
// lower then disagree; a minimum on a rounding tie (min = -max) gives -1.
// Clamp before the cast, which wraps (256 -> 0, -1 -> 255) and would
// decode one extreme as the other; no in-range value changes.
__device__ __forceinline__ uint8_t quant_level_u8(float q) {
  return (uint8_t)fminf(fmaxf(q, 0.0f), 255.0f);
}

// grid.y = chunk; writes 32B header (min,max float32) + payload
template <typename T>
__global__ void quantize_kernel(const T* __restrict__ x, size_t chunk,
                                int chunk_begin, size_t chunk_stride,
                                const uint32_t* __restrict__ scratch,
                                uint8_t* __restrict__ out) {
  const int c = chunk_begin + blockIdx.y;
  const float mn = ordered_to_f32(scratch[2 * c]);
  const float mx = ordered_to_f32(scratch[2 * c + 1]);
  float scale, lower, upper;
  quant_params(mn, mx, scale, lower, upper);

  uint8_t* __restrict__ dst = out + (size_t)c * chunk_stride;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float* hdr = reinterpret_cast<float*>(dst);
    hdr[0] = mn;
    hdr[1] = mx;
    // zero the header tail (bytes 8..31): the wire buffer is sent to
    // peers, so uninitialized bytes would leak GPU memory contents and
    // make the wire non-deterministic vs the zero-padded CPU oracle.
#pragma unroll
    for (int k = 2; k < 8; ++k) hdr[k] = 0.0f;
  }
  const T* __restrict__ src = x + (size_t)c * chunk;
  uint8_t* __restrict__ payload = dst + 32;
  // same reason for the padding behind the payload (bytes 32+chunk ..
  // chunk_stride, at most 31 of them): callers hand in torch.empty wires
  if (blockIdx.x == 0) {
    const size_t pad = chunk_stride - 32 - chunk;
    if (threadIdx.x < pad) payload[chunk + threadIdx.x] = 0;
  }

  // per-T width (measured, gpurun r2c9): 16-byte tensor-side loads win;
  // widening the u8 store granule beyond that costs ~1%
  constexpr int V = Vec16<T>::N;  // 4 (f32) / 8 (f16, bf16)
  using VT = Vec16<T>;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = chunk / V;
  const VT* sv = reinterpret_cast<const VT*>(src);
  for (size_t i = tid; i < nv; i += stride) {
    VT a = sv[i];
    uint8_t q[Vec16<T>::N];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float level = fminf(rintf(to_f(a.v[k]) * scale), upper);
      q[k] = quant_level_u8(level - lower);
    }
    if (V == 4)
      *reinterpret_cast<uint32_t*>(payload + i * 4) =
          *reinterpret_cast<uint32_t*>(q);
    else
      *reinterpret_cast<uint64_t*>(payload + i * 8) =
          *reinterpret_cast<uint64_t*>(q);
  }
  for (size_t i = nv * V + tid; i < chunk; i += stride) {
    float level = fminf(rintf(to_f(src[i]) * scale), upper);
    payload[i] = quant_level_u8(level - lower);
  }
}

template <typename T>
__global__ void dequantize_kernel(const uint8_t* __restrict__ in,
                                  size_t chunk, int chunk_begin,
                                  size_t chunk_stride, T* __restrict__ x) {
  const int c = chunk_begin + blockIdx.y;
  const uint8_t* __restrict__ src = in + (size_t)c * chunk_stride;
  const float* hdr = reinterpret_cast<const float*>(src);
  const float mn = hdr[0], mx = hdr[1];
  float scale, lower, upper;
  quant_params(mn, mx, scale, lower, upper);
  const float inv_scale = 1.0f / scale;

  const uint8_t* __restrict__ payload = src + 32;
  T* __restrict__ dst = x + (size_t)c * chunk;

  // per-dtype width (measured, gpurun r2c9): f32 wants V=4 (4-byte
  // payload load + one 16-byte store — V=16's four stores per lane cost
  // -43%); f16/bf16 want V=16 (one 16-byte payload load, two 16-byte
  // stores — +21% over V=8)
  constexpr int V = sizeof(T) == 4 ? 4 : 16;
  constexpr int OV = Vec16<T>::N;
  constexpr int NOUT = V / OV;
  using VT = Vec16<T>;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = chunk / V;
  VT* dv = reinterpret_cast<VT*>(dst);
  for (size_t i = tid; i < nv; i += stride) {
    alignas(16) uint8_t q[V];
    if (V == 4)
      *reinterpret_cast<uint32_t*>(q) =
          *reinterpret_cast<const uint32_t*>(payload + i * 4);
    else
      *reinterpret_cast<uint4*>(q) =
          *reinterpret_cast<const uint4*>(payload + i * 16);
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      VT out;
#pragma unroll
      for (int k = 0; k < OV; ++k)
        out.v[k] = from_f<T>(((float)q[o * OV + k] + lower) * inv_scale);
      dv[i * NOUT + o] = out;
    }
  }
  for (size_t i = nv * V + tid; i < chunk; i += stride)
    dst[i] = from_f<T>(((float)payload[i] + lower) * inv_scale);
}

// ---------------------------------------------------------------------------
// fused dequantize + chunk reduce (ByteGrad hot path).
//
// After the alltoall, the bucket's non-target chunks exist only as
// inputs to the reduction — materializing them through a full
// decompress pass and re-reading them in reduce_chunk wastes ~2 bucket
// passes of HBM traffic. This kernel reads the wire payloads directly
// (n_chunks x u8), dequantizes in registers and writes ONLY the target
// chunk. Values round through T between dequantize and accumulate so
// the result is BITWISE identical to dequantize_kernel +
// reduce_chunk_kernel (the CPU oracle and the python executor take that
// unfused chain).
// ---------------------------------------------------------------------------

#define DQR_MAX_CHUNKS 64

template <typename T>
__global__ void dequant_reduce_kernel(const uint8_t* __restrict__ in,
                                      size_t chunk, size_t chunk_stride,
                                      int num_chunks, float post_scale,
                                      T* __restrict__ dst /* target base */) {
  // no FMA contraction: for T=float the dequantized value must round
  // exactly as the unfused dequantize kernel's store did, or bitwise
  // parity with decompress+reduce breaks (memory-bound kernel — FMA
  // contributes nothing here anyway)
#pragma clang fp contract(off)
  // per-chunk quant params staged through LDS once per block
  __shared__ float s_lower[DQR_MAX_CHUNKS];
  __shared__ float s_inv_scale[DQR_MAX_CHUNKS];
  for (int c = threadIdx.x; c < num_chunks; c += blockDim.x) {
    const float* hdr =
        reinterpret_cast<const float*>(in + (size_t)c * chunk_stride);
    float scale, lower, upper;
    quant_params(hdr[0], hdr[1], scale, lower, upper);
    s_lower[c] = lower;
    s_inv_scale[c] = 1.0f / scale;
  }
  __syncthreads();

  // per-dtype width, same tradeoff as dequantize_kernel (measured
  // r2c9): f32 V=4, f16/bf16 V=16
  constexpr int V = sizeof(T) == 4 ? 4 : 16;
  constexpr int OV = Vec16<T>::N;       // elems per 16B output vector
  constexpr int NOUT = V / OV;          // output vectors per iteration
  using VT = Vec16<T>;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = chunk / V;
  VT* dv = reinterpret_cast<VT*>(dst);
  for (size_t i = tid; i < nv; i += stride) {
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int c = 0; c < num_chunks; ++c) {
      const uint8_t* payload = in + (size_t)c * chunk_stride + 32;
      alignas(16) uint8_t q[V];
      if (V == 4)
        *reinterpret_cast<uint32_t*>(q) =
            *reinterpret_cast<const uint32_t*>(payload + i * 4);
      else
        *reinterpret_cast<uint4*>(q) =
            *reinterpret_cast<const uint4*>(payload + i * 16);
      const float lower = s_lower[c], inv_scale = s_inv_scale[c];
#pragma unroll
      for (int k = 0; k < V; ++k)
        acc[k] += to_f(from_f<T>(((float)q[k] + lower) * inv_scale));
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      VT out;
#pragma unroll
      for (int k = 0; k < OV; ++k)
        out.v[k] = from_f<T>(acc[o * OV + k] * post_scale);
      dv[i * NOUT + o] = out;
    }
  }
  for (size_t i = nv * V + tid; i < chunk; i += stride) {
    float acc = 0.f;
    for (int c = 0; c < num_chunks; ++c) {
      const uint8_t* payload = in + (size_t)c * chunk_stride + 32;
      acc += to_f(from_f<T>(((float)payload[i] + s_lower[c])
                            * s_inv_scale[c]));
    }
    dst[i] = from_f<T>(acc * post_scale);
  }
}

// ---------------------------------------------------------------------------
// host-side launchers (extern "C", stream-passing; no syncs)
// ---------------------------------------------------------------------------

static inline int grid_for(size_t work_items) {
  size_t g = (work_items + BLOCK - 1) / BLOCK;
  if (g > MAX_GRID) g = MAX_GRID;
  if (g < 1) g = 1;
  return (int)g;
}

template <typename T, int OP>
static void launch_ew(void* x, const void* y, float f, size_t n,
                      hipStream_t stream) {
  int grid = grid_for(n / (2 * Vec16<T>::N) + 1);
  hipLaunchKernelGGL((ew_kernel<T, OP>), dim3(grid), dim3(BLOCK), 0, stream,
                     (T*)x, (const T*)y, f, n);
}

extern "C" {

// dtype: 0=f32, 1=f16, 2=bf16
void bagua_ew_launch(int op, int dtype, void* x, const void* y, float f,
                     size_t n, hipStream_t stream) {
  if (op == EW_AVERAGE) {
    switch (dtype) {
      case 0: launch_ew<float, EW_AVERAGE>(x, y, f, n, stream); break;
      case 1: launch_ew<__half, EW_AVERAGE>(x, y, f, n, stream); break;
      case 2: launch_ew<__hip_bfloat16, EW_AVERAGE>(x, y, f, n, stream); break;
    }
  } else if (op == EW_ADD) {
    switch (dtype) {
      case 0: launch_ew<float, EW_ADD>(x, y, f, n, stream); break;
      case 1: launch_ew<__half, EW_ADD>(x, y, f, n, stream); break;
      case 2: launch_ew<__hip_bfloat16, EW_ADD>(x, y, f, n, stream); break;
    }
  } else if (op == EW_SUB) {
    switch (dtype) {
      case 0: launch_ew<float, EW_SUB>(x, y, f, n, stream); break;
      case 1: launch_ew<__half, EW_SUB>(x, y, f, n, stream); break;
      case 2: launch_ew<__hip_bfloat16, EW_SUB>(x, y, f, n, stream); break;
    }
  } else if (op == EW_ADDMUL) {
    switch (dtype) {
      case 0: launch_ew<float, EW_ADDMUL>(x, y, f, n, stream); break;
      case 1: launch_ew<__half, EW_ADDMUL>(x, y, f, n, stream); break;
      case 2: launch_ew<__hip_bfloat16, EW_ADDMUL>(x, y, f, n, stream); break;
    }
  } else if (op == EW_DIV) {
    switch (dtype) {
      case 0: launch_ew<float, EW_DIV>(x, y, f, n, stream); break;
      case 1: launch_ew<__half, EW_DIV>(x, y, f, n, stream); break;
      case 2: launch_ew<__hip_bfloat16, EW_DIV>(x, y, f, n, stream); break;
    }
  }
}

void bagua_async_avg_launch(int dtype, void* x, const void* reduced,
                            const void* x_copy, float nranks, size_t n,
                            hipStream_t stream) {
  int grid = grid_for(n / 4 + 1);
  float inv_n = 1.0f / nranks;
  switch (dtype) {
    case 0:
      hipLaunchKernelGGL((async_avg_kernel<float>), dim3(grid), dim3(BLOCK),
                         0, stream, (float*)x, (const float*)reduced,
                         (const float*)x_copy, inv_n, n);
      break;
    case 1:
      hipLaunchKernelGGL((async_avg_kernel<__half>), dim3(grid), dim3(BLOCK),
                         0, stream, (__half*)x, (const __half*)reduced,
                         (const __half*)x_copy, inv_n, n);
      break;
    case 2:
      hipLaunchKernelGGL((async_avg_kernel<__hip_bfloat16>), dim3(grid),
                         dim3(BLOCK), 0, stream, (__hip_bfloat16*)x,
                         (const __hip_bfloat16*)reduced,
                         (const __hip_bfloat16*)x_copy, inv_n, n);
      break;
  }
}

void bagua_reduce_chunk_launch(int dtype, void* x, int num_chunks,
                               int target_chunk, int average, size_t chunk,
                               hipStream_t stream) {
  int grid = grid_for(chunk / 4 + 1);
  float post = average ? 1.0f / num_chunks : 1.0f;
  switch (dtype) {
    case 0:
      hipLaunchKernelGGL((reduce_chunk_kernel<float>), dim3(grid),
                         dim3(BLOCK), 0, stream, (float*)x, num_chunks,
                         target_chunk, post, chunk);
      break;
    case 1:
      hipLaunchKernelGGL((reduce_chunk_kernel<__half>), dim3(grid),
                         dim3(BLOCK), 0, stream, (__half*)x, num_chunks,
                         target_chunk, post, chunk);
      break;
    case 2:
      hipLaunchKernelGGL((reduce_chunk_kernel<__hip_bfloat16>), dim3(grid),
                         dim3(BLOCK), 0, stream, (__hip_bfloat16*)x,
                         num_chunks, target_chunk, post, chunk);
      break;
  }
}

// scratch: uint32[2*num_chunks_total]; out: chunked wire buffer
void bagua_compress_launch(int dtype, const void* x, uint8_t* out,
                           uint32_t* scratch, uint32_t* partials,
                           size_t chunk, size_t chunk_stride,
                           int num_chunks_total, int chunk_begin,
                           int chunk_count, hipStream_t stream) {
  int gx = grid_for(chunk / 8 + 1);
  if (gx > MINMAX_MAX_BLOCKS) gx = MINMAX_MAX_BLOCKS;
  dim3 grid(gx, chunk_count);
  switch (dtype) {
    case 0:
      hipLaunchKernelGGL((minmax_kernel<float>), grid, dim3(BLOCK), 0,
                         stream, (const float*)x, chunk, chunk_begin,
                         partials);
      hipLaunchKernelGGL(minmax_finalize_kernel, dim3(chunk_count),
                         dim3(BLOCK), 0, stream, partials, gx,
                         chunk_begin, scratch);
      hipLaunchKernelGGL((quantize_kernel<float>), grid, dim3(BLOCK), 0,
                         stream, (const float*)x, chunk, chunk_begin,
                         chunk_stride, scratch, out);
      break;
    case 1:
      hipLaunchKernelGGL((minmax_kernel<__half>), grid, dim3(BLOCK), 0,
                         stream, (const __half*)x, chunk, chunk_begin,
                         partials);
      hipLaunchKernelGGL(minmax_finalize_kernel, dim3(chunk_count),
                         dim3(BLOCK), 0, stream, partials, gx,
                         chunk_begin, scratch);
      hipLaunchKernelGGL((quantize_kernel<__half>), grid, dim3(BLOCK), 0,
                         stream, (const __half*)x, chunk, chunk_begin,
                         chunk_stride, scratch, out);
      break;
    case 2:
      hipLaunchKernelGGL((minmax_kernel<__hip_bfloat16>), grid, dim3(BLOCK),
                         0, stream, (const __hip_bfloat16*)x, chunk,
                         chunk_begin, partials);
      hipLaunchKernelGGL(minmax_finalize_kernel, dim3(chunk_count),
                         dim3(BLOCK), 0, stream, partials, gx,
                         chunk_begin, scratch);
      hipLaunchKernelGGL((quantize_kernel<__hip_bfloat16>), grid,
                         dim3(BLOCK), 0, stream, (const __hip_bfloat16*)x,
                         chunk, chunk_begin, chunk_stride, scratch, out);
      break;
  }
}

void bagua_decompress_launch(int dtype, const uint8_t* in, void* x,
                             size_t chunk, size_t chunk_stride,
                             int chunk_begin, int chunk_count,
                             hipStream_t stream) {
  int gx = grid_for(chunk / 8 + 1);
  if (gx > 512) gx = 512;
  dim3 grid(gx, chunk_count);
  switch (dtype) {
    case 0:
      hipLaunchKernelGGL((dequantize_kernel<float>), grid, dim3(BLOCK), 0,
                         stream, in, chunk, chunk_begin, chunk_stride,
                         (float*)x);
      break;
    case 1:
      hipLaunchKernelGGL((dequantize_kernel<__half>), grid, dim3(BLOCK), 0,
                         stream, in, chunk, chunk_begin, chunk_stride,
                         (__half*)x);
      break;
    case 2:
      hipLaunchKernelGGL((dequantize_kernel<__hip_bfloat16>), grid,
                         dim3(BLOCK), 0, stream, in, chunk, chunk_begin,
                         chunk_stride, (__hip_bfloat16*)x);
      break;
  }
}

// fused dequantize + reduce of all wire chunks into flat's target chunk
// (x points at the BUCKET base; target offset applied here)
void bagua_dequant_reduce_launch(int dtype, const uint8_t* in, void* x,
                                 size_t chunk, size_t chunk_stride,
                                 int num_chunks, int target_chunk,
                                 int average, hipStream_t stream) {
  float post_scale = average ? 1.0f / (float)num_chunks : 1.0f;
  int grid = grid_for(chunk / 16 + 1);
  switch (dtype) {
    case 0:
      hipLaunchKernelGGL((dequant_reduce_kernel<float>), dim3(grid),
                         dim3(BLOCK), 0, stream, in, chunk, chunk_stride,
                         num_chunks, post_scale,
                         (float*)x + (size_t)target_chunk * chunk);
      break;
    case 1:
      hipLaunchKernelGGL((dequant_reduce_kernel<__half>), dim3(grid),
                         dim3(BLOCK), 0, stream, in, chunk, chunk_stride,
                         num_chunks, post_scale,
                         (__half*)x + (size_t)target_chunk * chunk);
      break;
    case 2:
      hipLaunchKernelGGL((dequant_reduce_kernel<__hip_bfloat16>),
                         dim3(grid), dim3(BLOCK), 0, stream, in, chunk,
                         chunk_stride, num_chunks, post_scale,
                         (__hip_bfloat16*)x + (size_t)target_chunk * chunk);
      break;
  }
}

}  // extern "C"

// ---------------------------------------------------------------------------
// fused optimizer steps (f32 master weights) — one pass over the flat
// param group: grad transform + momentum/variance update + weight update
// in a single memory-bound kernel instead of the 3-5 launches of a
// generic foreach optimizer. MI355X-native addition (the reference fused
// by contiguity only; north-star asks for the fused step as a HIP
// kernel).
// ---------------------------------------------------------------------------

// Per-element arithmetic, one function per optimizer: the flat and the
// segmented kernels call it on their vector and scalar paths alike. Every
// fused multiply-add is written out and contraction is switched off, so
// the rounding does not depend on what the compiler makes of the code
// around a call: that is what keeps all those paths bitwise equal. (Left
// to the compiler, momentum * m + (1 - dampening) * grad came out as three
// different instruction sequences in three call sites.)

// SGD with momentum/dampening/nesterov/weight-decay (torch semantics).
// m is read only when momentum_initialized, written when momentum != 0.
__device__ __forceinline__ void sgd_update(float& w, float g, float& m,
                                           float lr, float momentum,
                                           float dampening,
                                           float weight_decay, int nesterov,
                                           int momentum_initialized) {
#pragma clang fp contract(off)
  float grad = fmaf(weight_decay, w, g);
  float upd = grad;
  if (momentum != 0.f) {
    float buf = momentum_initialized
                    ? fmaf(1.f - dampening, grad, momentum * m)
                    : grad;
    m = buf;
    upd = nesterov ? fmaf(momentum, buf, grad) : buf;
  }
  w = fmaf(-lr, upd, w);
}

// Adam / AdamW (torch semantics, bias-corrected)
__device__ __forceinline__ void adam_update(float& w, float g, float& m,
                                            float& v, float lr, float beta1,
                                            float beta2,
                                            float one_minus_beta1,
                                            float one_minus_beta2, float eps,
                                            float weight_decay, int adamw,
                                            float inv_bc1,
                                            float inv_sqrt_bc2) {
#pragma clang fp contract(off)
  float param = w;
  float grad = g;
  if (adamw)
    param *= fmaf(-lr, weight_decay, 1.f);
  else
    grad = fmaf(weight_decay, param, grad);
  float mi = fmaf(beta1, m, one_minus_beta1 * grad);
  float vi = fmaf(beta2, v, one_minus_beta2 * grad * grad);
  m = mi;
  v = vi;
  float denom = fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
  w = param - lr * inv_bc1 * mi / denom;
}

extern "C" {

// SGD with momentum/dampening/nesterov/weight-decay (torch semantics)
__global__ void fused_sgd_kernel(float* __restrict__ p,
                                 const float* __restrict__ g,
                                 float* __restrict__ m, float lr,
                                 float momentum, float dampening,
                                 float weight_decay, int nesterov,
                                 int momentum_initialized, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // two float4 per lane per iteration (32 B accesses, +5-9% on the RMW
  // mix per the elementwise measurements)
  const size_t nv = n / 8;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  for (size_t i = tid; i < nv; i += stride) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const size_t idx = 2 * i + j;
      float4 pv = p4[idx], gv = g4[idx];
      float4 mv = momentum != 0.f ? m4[idx] : make_float4(0, 0, 0, 0);
      float* pp = &pv.x;
      const float* gg = &gv.x;
      float* mm = &mv.x;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        sgd_update(pp[k], gg[k], mm[k], lr, momentum, dampening,
                   weight_decay, nesterov, momentum_initialized);
      p4[idx] = pv;
      if (momentum != 0.f) m4[idx] = mv;
    }
  }
  for (size_t i = nv * 8 + tid; i < n; i += stride) {
    float w = p[i];
    float mi = momentum != 0.f && momentum_initialized ? m[i] : 0.f;
    sgd_update(w, g[i], mi, lr, momentum, dampening, weight_decay, nesterov,
               momentum_initialized);
    p[i] = w;
    if (momentum != 0.f) m[i] = mi;
  }
}

// Adam / AdamW (torch semantics, bias-corrected). 1 - beta and the bias
// corrections come from the host, formed in double and cast once: in f32
// 1.f - 0.999f is off by 1.3e-5 relative (the subtraction cancels), which
// sqrt(v) carries into every update.
__global__ void fused_adam_kernel(float* __restrict__ p,
                                  const float* __restrict__ g,
                                  float* __restrict__ m,
                                  float* __restrict__ v, float lr,
                                  float beta1, float beta2,
                                  float one_minus_beta1,
                                  float one_minus_beta2, float eps,
                                  float weight_decay, int adamw,
                                  float bias_correction1,
                                  float bias_correction2, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float inv_bc1 = 1.f / bias_correction1;
  const float inv_sqrt_bc2 = rsqrtf(bias_correction2);
  // vectorized: two float4 per lane per array (32 B accesses; the
  // scalar form measured 5.0 TB/s vs the ~7 TB/s RMW ceiling)
  const size_t nv = n / 8;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  for (size_t i = tid; i < nv; i += stride) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const size_t idx = 2 * i + j;
      float4 pv = p4[idx], gv = g4[idx], mv = m4[idx], vv = v4[idx];
      float* pp = &pv.x;
      float* gg = &gv.x;
      float* mm = &mv.x;
      float* uu = &vv.x;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        adam_update(pp[k], gg[k], mm[k], uu[k], lr, beta1, beta2,
                    one_minus_beta1, one_minus_beta2, eps, weight_decay,
                    adamw, inv_bc1, inv_sqrt_bc2);
      p4[idx] = pv;
      m4[idx] = mv;
      v4[idx] = vv;
    }
  }
  for (size_t i = nv * 8 + tid; i < n; i += stride) {
    adam_update(p[i], g[i], m[i], v[i], lr, beta1, beta2, one_minus_beta1,
                one_minus_beta2, eps, weight_decay, adamw, inv_bc1,
                inv_sqrt_bc2);
  }
}

void bagua_fused_sgd_launch(float* p, const float* g, float* m, float lr,
                            float momentum, float dampening,
                            float weight_decay, int nesterov,
                            int momentum_initialized, size_t n,
                            hipStream_t stream) {
  int grid = grid_for(n / 8 + 1);
  hipLaunchKernelGGL(fused_sgd_kernel, dim3(grid), dim3(BLOCK), 0, stream,
                     p, g, m, lr, momentum, dampening, weight_decay,
                     nesterov, momentum_initialized, n);
}


// bf16 weights + fp32 master + bf16 grads: the pure-bf16 training path
// (fp32 master keeps SGD exact; bf16 params keep fwd/bwd and the grad
// allreduce at half the bytes)
__global__ void fused_sgd_mixed_kernel(__hip_bfloat16* __restrict__ p,
                                       const __hip_bfloat16* __restrict__ g,
                                       float* __restrict__ master,
                                       float* __restrict__ m, float lr,
                                       float momentum, float dampening,
                                       float weight_decay, int nesterov,
                                       int momentum_initialized, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // 8 elements per lane: one 16 B bf16 load/store + two float4 master/
  // momentum accesses (the scalar form paid the 2-2.5x slow bf16
  // scalar-load path on the flagship pure-bf16 bench)
  const size_t nv = n / 8;
  using BV = Vec16<__hip_bfloat16>;  // 8 bf16
  BV* p8 = reinterpret_cast<BV*>(p);
  const BV* g8 = reinterpret_cast<const BV*>(g);
  float4* ma4 = reinterpret_cast<float4*>(master);
  float4* m4 = reinterpret_cast<float4*>(m);
  for (size_t i = tid; i < nv; i += stride) {
    BV gv = g8[i];
    BV pv;
    float4 w[2] = {ma4[2 * i], ma4[2 * i + 1]};
    float4 mb[2];
    if (momentum != 0.f && momentum_initialized) {
      mb[0] = m4[2 * i];
      mb[1] = m4[2 * i + 1];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float* ww = &w[k / 4].x;
      float* mm = &mb[k / 4].x;
      sgd_update(ww[k % 4], __bfloat162float(gv.v[k]), mm[k % 4], lr,
                 momentum, dampening, weight_decay, nesterov,
                 momentum_initialized);
      pv.v[k] = __float2bfloat16(ww[k % 4]);
    }
    ma4[2 * i] = w[0];
    ma4[2 * i + 1] = w[1];
    if (momentum != 0.f) {
      m4[2 * i] = mb[0];
      m4[2 * i + 1] = mb[1];
    }
    p8[i] = pv;
  }
  for (size_t i = nv * 8 + tid; i < n; i += stride) {
    float w = master[i];
    float mi = momentum != 0.f && momentum_initialized ? m[i] : 0.f;
    sgd_update(w, __bfloat162float(g[i]), mi, lr, momentum, dampening,
               weight_decay, nesterov, momentum_initialized);
    master[i] = w;
    if (momentum != 0.f) m[i] = mi;
    p[i] = __float2bfloat16(w);
  }
}

void bagua_fused_sgd_mixed_launch(void* p, const void* g, float* master,
                                  float* m, float lr, float momentum,
                                  float dampening, float weight_decay,
                                  int nesterov, int momentum_initialized,
                                  size_t n, hipStream_t stream) {
  int grid = grid_for(n / 8 + 1);
  hipLaunchKernelGGL(fused_sgd_mixed_kernel, dim3(grid), dim3(BLOCK), 0,
                     stream, (__hip_bfloat16*)p, (const __hip_bfloat16*)g,
                     master, m, lr, momentum, dampening, weight_decay,
                     nesterov, momentum_initialized, n);
}

void bagua_fused_adam_launch(float* p, const float* g, float* m, float* v,
                             float lr, float beta1, float beta2,
                             float one_minus_beta1, float one_minus_beta2,
                             float eps, float weight_decay, int adamw,
                             float bc1, float bc2, size_t n,
                             hipStream_t stream) {
  int grid = grid_for(n / 8 + 1);
  hipLaunchKernelGGL(fused_adam_kernel, dim3(grid), dim3(BLOCK), 0, stream,
                     p, g, m, v, lr, beta1, beta2, one_minus_beta1,
                     one_minus_beta2, eps, weight_decay, adamw, bc1, bc2, n);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// segmented fused steps: weights, master and optimizer state stay flat and
// are accessed exactly as above; only the gradient is read where it lives
// (a bucket view, a fresh autograd tensor, or nowhere at all), through a
// table of segments {grad, begin, numel} in flat-element space. That saves
// the gather of every gradient into a flat copy before each step.
//
// The table travels by value in the kernel arguments (no device-side
// table, no copy, nothing to allocate: the step stays graph-capturable);
// more than SEG_CAP segments take several launches. A launch covers the
// flat range [begin of its first segment, end of its last) and grid-
// strides over the 8-element flat vectors that overlap it. A vector that
// lies inside one segment and inside the range takes the vector path of
// the flat kernels, with the gradient vector-loaded when its address is
// 16-byte aligned and element by element otherwise. A vector that
// straddles two segments or the range's edge goes element-wise; there are
// at most two of those per segment. A null grad pointer is a zero
// gradient.
// ---------------------------------------------------------------------------

#define SEG_CAP 128  // 128 x 24 B + the op's scalars < 4 KB of kernel args

struct GradSeg {
  const void* grad;  // null: zero gradient
  size_t begin;      // flat element offset
  size_t numel;      // > 0
};

struct SegTable {
  GradSeg seg[SEG_CAP];  // contiguous in flat space, ascending
  int count;
};

// A gradient pointer comes out of the table, so the compiler cannot see
// that it points to global memory, as it can for a kernel argument. Saying
// so keeps the gradient loads global loads and not flat ones. Gradients
// are read as raw elements: float, or the 16 bits of a bf16.
#define GLOBAL_AS __attribute__((address_space(1)))
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float grad_to_f(float v) { return v; }
__device__ __forceinline__ float grad_to_f(unsigned short bf16_bits) {
  return __uint_as_float((unsigned)bf16_bits << 16);
}

__device__ __forceinline__ void load_grad8(const float GLOBAL_AS* g,
                                           float (&out)[8]) {
  const f32x4_t a = reinterpret_cast<const f32x4_t GLOBAL_AS*>(g)[0];
  const f32x4_t b = reinterpret_cast<const f32x4_t GLOBAL_AS*>(g)[1];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    out[k] = a[k];
    out[4 + k] = b[k];
  }
}

__device__ __forceinline__ void load_grad8(const unsigned short GLOBAL_AS* g,
                                           float (&out)[8]) {
  const u16x8_t a = *reinterpret_cast<const u16x8_t GLOBAL_AS*>(g);
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = grad_to_f(a[k]);
}

// f32 weights, f32 grads
struct SgdSegOp {
  using grad_t = float;
  float* p;
  float* m;
  float lr, momentum, dampening, weight_decay;
  int nesterov, momentum_initialized;

  // Flat vector i8 (elements 8*i8 .. 8*i8+7, all inside the range) in two
  // halves, so that the kernel can issue the flat loads before it branches
  // on where the gradient is: load(), then finish() with the gradient.
  struct Vec {
    float4 w[2], mb[2];
  };

  __device__ __forceinline__ void load(size_t i8, Vec& s) const {
    const float4* p4 = reinterpret_cast<const float4*>(p) + 2 * i8;
    const float4* m4 = reinterpret_cast<const float4*>(m) + 2 * i8;
    s.w[0] = p4[0];
    s.w[1] = p4[1];
    if (momentum != 0.f && momentum_initialized) {
      s.mb[0] = m4[0];
      s.mb[1] = m4[1];
    }
  }

  __device__ __forceinline__ void finish(size_t i8, Vec& s,
                                         const float (&g)[8]) const {
    float4* p4 = reinterpret_cast<float4*>(p) + 2 * i8;
    float4* m4 = reinterpret_cast<float4*>(m) + 2 * i8;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      sgd_update((&s.w[k / 4].x)[k % 4], g[k], (&s.mb[k / 4].x)[k % 4], lr,
                 momentum, dampening, weight_decay, nesterov,
                 momentum_initialized);
    p4[0] = s.w[0];
    p4[1] = s.w[1];
    if (momentum != 0.f) {
      m4[0] = s.mb[0];
      m4[1] = s.mb[1];
    }
  }

  __device__ __forceinline__ void one(size_t i, float g) const {
    float w = p[i];
    float mi = momentum != 0.f && momentum_initialized ? m[i] : 0.f;
    sgd_update(w, g, mi, lr, momentum, dampening, weight_decay, nesterov,
               momentum_initialized);
    p[i] = w;
    if (momentum != 0.f) m[i] = mi;
  }
};

// bf16 weights + f32 master, bf16 grads
struct SgdMixedSegOp {
  using grad_t = unsigned short;  // bf16 bits
  __hip_bfloat16* p;
  float* master;
  float* m;
  float lr, momentum, dampening, weight_decay;
  int nesterov, momentum_initialized;

  struct Vec {
    float4 w[2], mb[2];
  };

  __device__ __forceinline__ void load(size_t i8, Vec& s) const {
    const float4* ma4 = reinterpret_cast<const float4*>(master) + 2 * i8;
    const float4* m4 = reinterpret_cast<const float4*>(m) + 2 * i8;
    s.w[0] = ma4[0];
    s.w[1] = ma4[1];
    if (momentum != 0.f && momentum_initialized) {
      s.mb[0] = m4[0];
      s.mb[1] = m4[1];
    }
  }

  __device__ __forceinline__ void finish(size_t i8, Vec& s,
                                         const float (&g)[8]) const {
    float4* ma4 = reinterpret_cast<float4*>(master) + 2 * i8;
    float4* m4 = reinterpret_cast<float4*>(m) + 2 * i8;
    Vec16<__hip_bfloat16> pv;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sgd_update((&s.w[k / 4].x)[k % 4], g[k], (&s.mb[k / 4].x)[k % 4], lr,
                 momentum, dampening, weight_decay, nesterov,
                 momentum_initialized);
      pv.v[k] = __float2bfloat16((&s.w[k / 4].x)[k % 4]);
    }
    ma4[0] = s.w[0];
    ma4[1] = s.w[1];
    if (momentum != 0.f) {
      m4[0] = s.mb[0];
      m4[1] = s.mb[1];
    }
    reinterpret_cast<Vec16<__hip_bfloat16>*>(p)[i8] = pv;
  }

  __device__ __forceinline__ void one(size_t i, float g) const {
    float w = master[i];
    float mi = momentum != 0.f && momentum_initialized ? m[i] : 0.f;
    sgd_update(w, g, mi, lr, momentum, dampening, weight_decay, nesterov,
               momentum_initialized);
    master[i] = w;
    if (momentum != 0.f) m[i] = mi;
    p[i] = __float2bfloat16(w);
  }
};

// f32 weights, f32 grads
struct AdamSegOp {
  using grad_t = float;
  float* p;
  float* m;
  float* v;
  float lr, beta1, beta2, one_minus_beta1, one_minus_beta2, eps;
  float weight_decay, bias_correction1, bias_correction2;
  int adamw;

  struct Vec {
    float4 w[2], mb[2], vb[2];
  };

  __device__ __forceinline__ void load(size_t i8, Vec& s) const {
    const float4* p4 = reinterpret_cast<const float4*>(p) + 2 * i8;
    const float4* m4 = reinterpret_cast<const float4*>(m) + 2 * i8;
    const float4* v4 = reinterpret_cast<const float4*>(v) + 2 * i8;
    s.w[0] = p4[0];
    s.w[1] = p4[1];
    s.mb[0] = m4[0];
    s.mb[1] = m4[1];
    s.vb[0] = v4[0];
    s.vb[1] = v4[1];
  }

  __device__ __forceinline__ void finish(size_t i8, Vec& s,
                                         const float (&g)[8]) const {
    float4* p4 = reinterpret_cast<float4*>(p) + 2 * i8;
    float4* m4 = reinterpret_cast<float4*>(m) + 2 * i8;
    float4* v4 = reinterpret_cast<float4*>(v) + 2 * i8;
    // formed on the device, as in fused_adam_kernel
    const float inv_bc1 = 1.f / bias_correction1;
    const float inv_sqrt_bc2 = rsqrtf(bias_correction2);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      adam_update((&s.w[k / 4].x)[k % 4], g[k], (&s.mb[k / 4].x)[k % 4],
                  (&s.vb[k / 4].x)[k % 4], lr, beta1, beta2,
                  one_minus_beta1, one_minus_beta2, eps, weight_decay, adamw,
                  inv_bc1, inv_sqrt_bc2);
    p4[0] = s.w[0];
    p4[1] = s.w[1];
    m4[0] = s.mb[0];
    m4[1] = s.mb[1];
    v4[0] = s.vb[0];
    v4[1] = s.vb[1];
  }

  __device__ __forceinline__ void one(size_t i, float g) const {
    const float inv_bc1 = 1.f / bias_correction1;
    const float inv_sqrt_bc2 = rsqrtf(bias_correction2);
    adam_update(p[i], g, m[i], v[i], lr, beta1, beta2, one_minus_beta1,
                one_minus_beta2, eps, weight_decay, adamw, inv_bc1,
                inv_sqrt_bc2);
  }
};

template <typename Op>
__global__ void __launch_bounds__(BLOCK)
fused_segments_kernel(Op op, SegTable tab) {
  using G = typename Op::grad_t;
  // the table is indexed per lane below, so it is staged in LDS first
  __shared__ size_t s_begin[SEG_CAP + 1];
  __shared__ const G* s_grad[SEG_CAP];
  const int count = tab.count;
  if ((int)threadIdx.x < count) {
    const GradSeg sg = tab.seg[threadIdx.x];
    s_begin[threadIdx.x] = sg.begin;
    s_grad[threadIdx.x] = static_cast<const G*>(sg.grad);
    if ((int)threadIdx.x == count - 1) s_begin[count] = sg.begin + sg.numel;
  }
  __syncthreads();
  const size_t lo = s_begin[0], hi = s_begin[count];
  const size_t v_end = (hi + 7) / 8;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // current segment [sb, se), kept across iterations: the search runs
  // again only when a lane's next vector has left it
  int s = 0;
  size_t sb = lo, se = s_begin[1];
  const G* sg = s_grad[0];
  for (size_t i8 = lo / 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
       i8 < v_end; i8 += stride) {
    const size_t i0 = i8 * 8;
    const size_t first = i0 > lo ? i0 : lo;  // first element in range
    if (first >= se) {
      int a = s + 1, b = count - 1;  // last segment with begin <= first
      while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (s_begin[mid] <= first) a = mid; else b = mid - 1;
      }
      s = a;
      sb = s_begin[s];
      se = s_begin[s + 1];
      sg = s_grad[s];
    }
    if (i0 >= lo && i0 + 8 <= se) {  // inside the range and one segment
      // flat loads first: they are then in flight while the gradient's
      // are, whichever branch below loads it
      typename Op::Vec st;
      op.load(i8, st);
      float g[8];
      if (sg == nullptr) {
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = 0.f;
      } else {
        const G GLOBAL_AS* gp = (const G GLOBAL_AS*)sg + (i0 - sb);
        if (((uintptr_t)gp & 15) == 0) {
          load_grad8(gp, g);
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) g[k] = grad_to_f(gp[k]);
        }
      }
      op.finish(i8, st, g);
    } else {
      // element by element; t walks on from the current segment
      int t = s;
      const size_t last = i0 + 8 < hi ? i0 + 8 : hi;
      for (size_t i = first; i < last; ++i) {
        while (i >= s_begin[t + 1]) ++t;
        const G GLOBAL_AS* gp = (const G GLOBAL_AS*)s_grad[t];
        op.one(i, gp != nullptr ? grad_to_f(gp[i - s_begin[t]]) : 0.f);
      }
    }
  }
}

// launches over consecutive runs of at most SEG_CAP segments
template <typename Op>
static void launch_segments(const Op& op, const void* const* grads,
                            const size_t* begins, const size_t* numels,
                            size_t count, hipStream_t stream) {
  for (size_t base = 0; base < count; base += SEG_CAP) {
    SegTable tab;
    tab.count = (int)(count - base < SEG_CAP ? count - base : SEG_CAP);
    for (int k = 0; k < tab.count; ++k)
      tab.seg[k] = GradSeg{grads[base + k], begins[base + k],
                           numels[base + k]};
    const size_t lo = tab.seg[0].begin;
    const size_t hi = tab.seg[tab.count - 1].begin +
                      tab.seg[tab.count - 1].numel;
    const int grid = grid_for((hi + 7) / 8 - lo / 8);
    hipLaunchKernelGGL((fused_segments_kernel<Op>), dim3(grid), dim3(BLOCK),
                       0, stream, op, tab);
  }
}

extern "C" {

// Segment k covers flat elements [begins[k], begins[k] + numels[k]); the
// segments are non-empty, ascending and contiguous (the caller checks).

void bagua_fused_sgd_segments_launch(float* p, float* m, float lr,
                                     float momentum, float dampening,
                                     float weight_decay, int nesterov,
                                     int momentum_initialized,
                                     const void* const* grads,
                                     const size_t* begins,
                                     const size_t* numels, size_t count,
                                     hipStream_t stream) {
  const SgdSegOp op{p, m, lr, momentum, dampening, weight_decay, nesterov,
                    momentum_initialized};
  launch_segments(op, grads, begins, numels, count, stream);
}

void bagua_fused_sgd_mixed_segments_launch(
    void* p, float* master, float* m, float lr, float momentum,
    float dampening, float weight_decay, int nesterov,
    int momentum_initialized, const void* const* grads, const size_t* begins,
    const size_t* numels, size_t count, hipStream_t stream) {
  const SgdMixedSegOp op{(__hip_bfloat16*)p, master, m, lr, momentum,
                         dampening, weight_decay, nesterov,
                         momentum_initialized};
  launch_segments(op, grads, begins, numels, count, stream);
}

void bagua_fused_adam_segments_launch(
    float* p, float* m, float* v, float lr, float beta1, float beta2,
    float one_minus_beta1, float one_minus_beta2, float eps,
    float weight_decay, int adamw, float bc1, float bc2,
    const void* const* grads, const size_t* begins, const size_t* numels,
    size_t count, hipStream_t stream) {
  const AdamSegOp op{p, m, v, lr, beta1, beta2, one_minus_beta1,
                     one_minus_beta2, eps, weight_decay, bc1, bc2, adamw};
  launch_segments(op, grads, begins, numels, count, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// p2p alltoall support: cross-GPU flag barrier over xGMI.
//
// The 8-GPU MI355X node is FULLY CONNECTED point-to-point (7 links/GPU),
// so a one-hop alltoall is: every rank pulls its chunk from each peer's
// exported send buffer. Ordering needs a device-side barrier — IPC
// events re-recorded every round race (a peer's wait can capture the
// previous recording), so ranks rendezvous on a monotonically increasing
// sequence number in FINE-GRAINED peer-visible memory instead:
//   arrive: write seq into MY slot of every peer's flag array
//   wait:   spin until every slot of MY flag array reaches seq
// One wave handles all peers (nranks <= 64 by construction).
// ---------------------------------------------------------------------------

__global__ void p2p_barrier_kernel(
    unsigned long long* const* __restrict__ peer_flags,  // [nranks] ptrs
    volatile unsigned long long* __restrict__ my_flags,  // [nranks]
    int rank, int nranks, unsigned long long seq) {
  const int p = threadIdx.x;
  if (p >= nranks) return;
  // make every prior write to my send buffer visible system-wide before
  // announcing arrival
  __threadfence_system();
  volatile unsigned long long* slot =
      (volatile unsigned long long*)(peer_flags[p]) + rank;
  *slot = seq;
  __threadfence_system();
  while (my_flags[p] < seq) {
    __builtin_amdgcn_s_sleep(8);
  }
  __threadfence_system();
}

extern "C" void bagua_p2p_barrier_launch(void* peer_flags_dev_array,
                                         void* my_flags, int rank,
                                         int nranks,
                                         unsigned long long seq,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, stream,
                     (unsigned long long* const*)peer_flags_dev_array,
                     (volatile unsigned long long*)my_flags, rank, nranks,
                     seq);
}
