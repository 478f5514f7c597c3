// CDNA4 (gfx950) kernels for index-based MoE routing.
//
// The dense GShard path moves tokens with einsums over a
// (tokens, experts, capacity) tensor that holds k non-zeros per token.
// These kernels work from integer routing indices instead:
//
//   assign_slots  queue position of each token at its chosen expert
//                 (== cumsum(one_hot) - 1 gathered at the choice), the
//                 per-expert counts, and the inverse map src[row]=token
//   gather_rows   out[r,:] = src[r] >= 0 ? scale(r) * x[src[r],:] : 0
//   combine_rows  out[s,:] = sum_j w[j,s] * eo[dest[j,s],:]
//   row_dot       gw[j,s]  = <g[s,:], eo[dest[j,s],:]>
//
// Design:
//  * no float atomics and a fixed reduction order everywhere, so every
//    result is bitwise reproducible; the only atomics are integer adds
//    into an LDS histogram, which commute;
//  * no inter-workgroup communication: slot assignment is three plain
//    launches (per-block histogram, single-block exclusive scan of the
//    block histograms, per-block ranking);
//  * row kernels are pure data movement: one 64-lane wave per row, 16 B
//    per lane when rows are 16-byte aligned, f32 math for f16/bf16 rows,
//    weights always f32; row offsets in size_t.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#define MOE_BLOCK 256
#define MOE_WAVE 64
#define MOE_WAVES (MOE_BLOCK / MOE_WAVE)
#define MOE_MAX_GRID 16384

namespace {

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

template <typename T> struct alignas(16) Vec16 {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

// ---------------------------------------------------------------------------
// slot assignment
// ---------------------------------------------------------------------------

// pass 1: hist[b][e] = tokens of block b choosing expert e
__global__ void moe_hist_kernel(const int* __restrict__ expert, int S, int E,
                                int* __restrict__ hist) {
  extern __shared__ int lds[];
  for (int e = threadIdx.x; e < E; e += MOE_BLOCK) lds[e] = 0;
  __syncthreads();
  const int t = blockIdx.x * MOE_BLOCK + threadIdx.x;
  if (t < S) {
    const int e = expert[t];
    if (e >= 0 && e < E) atomicAdd(&lds[e], 1);
  }
  __syncthreads();
  int* row = hist + (size_t)blockIdx.x * E;
  for (int e = threadIdx.x; e < E; e += MOE_BLOCK) row[e] = lds[e];
}

// pass 2 (one block): exclusive scan of hist over blocks, per expert, in
// place; adds base; writes the totals to counts
__global__ void moe_scan_kernel(int* __restrict__ hist, int nblocks, int E,
                                const int* __restrict__ base,
                                int* __restrict__ counts) {
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    const int b0 = base ? base[e] : 0;
    int run = 0;
    for (int b = 0; b < nblocks; ++b) {
      int* p = hist + (size_t)b * E + e;
      const int c = *p;
      *p = run + b0;
      run += c;
    }
    counts[e] = run;
  }
}

// pass 3: rank of every token among the earlier tokens of its expert.
// Inside a wave: ballot over the lanes sharing the expert, popcount of
// the lower lanes. Across the waves of the block: an LDS counter per
// expert (seeded with the block's scanned offset), advanced by one wave
// after the other so token order is kept.
__global__ void moe_rank_kernel(const int* __restrict__ expert, int S, int E,
                                int capacity, const int* __restrict__ offs,
                                int* __restrict__ slot,
                                int* __restrict__ src) {
  extern __shared__ int cnt[];
  const int* row = offs + (size_t)blockIdx.x * E;
  for (int e = threadIdx.x; e < E; e += MOE_BLOCK) cnt[e] = row[e];
  __syncthreads();

  const int t = blockIdx.x * MOE_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (MOE_WAVE - 1);
  const int wave = threadIdx.x / MOE_WAVE;
  const int e = t < S ? expert[t] : -1;
  const bool valid = e >= 0 && e < E;

  int rank = 0, group = 0;
  bool last = false;
  unsigned long long todo = __ballot(valid);
  while (todo) {  // wave-uniform: one round per distinct expert
    const int leader = __ffsll((long long)todo) - 1;
    const int e0 = __shfl(e, leader, MOE_WAVE);
    const bool mine = valid && e == e0;
    const unsigned long long m = __ballot(mine);
    if (mine) {
      rank = __popcll(m & ((1ull << lane) - 1ull));
      group = __popcll(m);
      last = lane == 63 - __clzll((long long)m);
    }
    todo &= ~m;
  }

  int pos = -1;
  for (int w = 0; w < MOE_WAVES; ++w) {
    if (wave == w && valid) pos = cnt[e] + rank;
    if (wave == w && last) cnt[e] += group;
    __syncthreads();
  }

  if (t < S) {
    slot[t] = pos;
    if (valid && pos >= 0 && pos < capacity)
      src[(size_t)e * capacity + pos] = t;
  }
}

// ---------------------------------------------------------------------------
// row kernels: one wave per row, grid-stride over rows
// ---------------------------------------------------------------------------

// weight of the choice that sent token s to row r
__device__ __forceinline__ float row_scale(const float* __restrict__ w,
                                           const int* __restrict__ dest,
                                           int k, int S, int s, size_t r) {
  if (!w) return 1.f;
  int j = 0;
  if (k == 2 && (size_t)(long long)dest[s] != r) j = 1;
  return w[(size_t)j * S + s];
}

template <typename T, bool VEC>
__global__ void moe_gather_rows_kernel(const T* __restrict__ x,
                                       const int* __restrict__ src,
                                       T* __restrict__ out,
                                       const float* __restrict__ w,
                                       const int* __restrict__ dest, int k,
                                       int S, size_t R, int M) {
  constexpr int V = Vec16<T>::N;
  using VT = Vec16<T>;
  const int lane = threadIdx.x & (MOE_WAVE - 1);
  const size_t wave0 = (size_t)blockIdx.x * MOE_WAVES + threadIdx.x / MOE_WAVE;
  const size_t nwaves = (size_t)gridDim.x * MOE_WAVES;
  for (size_t r = wave0; r < R; r += nwaves) {
    const int s = src[r];
    const bool live = s >= 0 && s < S;
    const float sc = live ? row_scale(w, dest, k, S, s, r) : 0.f;
    const T* xr = x + (size_t)(live ? s : 0) * M;
    T* orow = out + r * M;
    if (VEC) {
      const int nv = M / V;
      const VT* xv = reinterpret_cast<const VT*>(xr);
      VT* ov = reinterpret_cast<VT*>(orow);
      for (int i = lane; i < nv; i += MOE_WAVE) {
        VT a;
        if (live) {
          a = xv[i];
          if (w) {
#pragma unroll
            for (int q = 0; q < V; ++q)
              a.v[q] = from_f<T>(sc * to_f(a.v[q]));
          }
        } else {
#pragma unroll
          for (int q = 0; q < V; ++q) a.v[q] = from_f<T>(0.f);
        }
        ov[i] = a;
      }
    } else {
      for (int i = lane; i < M; i += MOE_WAVE) {
        T a = from_f<T>(0.f);
        if (live) a = w ? from_f<T>(sc * to_f(xr[i])) : xr[i];
        orow[i] = a;
      }
    }
  }
}

template <typename T, bool VEC, int K>
__global__ void moe_combine_rows_kernel(const T* __restrict__ eo,
                                        const int* __restrict__ dest,
                                        T* __restrict__ out,
                                        const float* __restrict__ w, int S,
                                        size_t R, int M) {
  constexpr int V = Vec16<T>::N;
  using VT = Vec16<T>;
  const int lane = threadIdx.x & (MOE_WAVE - 1);
  const size_t wave0 = (size_t)blockIdx.x * MOE_WAVES + threadIdx.x / MOE_WAVE;
  const size_t nwaves = (size_t)gridDim.x * MOE_WAVES;
  for (size_t s = wave0; s < (size_t)S; s += nwaves) {
    const T* er[K];
    float sc[K];
    bool live[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int d = dest[(size_t)j * S + s];
      live[j] = d >= 0 && (size_t)d < R;
      sc[j] = live[j] ? (w ? w[(size_t)j * S + s] : 1.f) : 0.f;
      er[j] = eo + (size_t)(live[j] ? d : 0) * M;
    }
    T* orow = out + s * M;
    if (VEC) {
      const int nv = M / V;
      VT* ov = reinterpret_cast<VT*>(orow);
      for (int i = lane; i < nv; i += MOE_WAVE) {
        float acc[V];
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (live[j]) {
            const VT a = reinterpret_cast<const VT*>(er[j])[i];
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] += sc[j] * to_f(a.v[q]);
          }
        }
        VT o;
#pragma unroll
        for (int q = 0; q < V; ++q) o.v[q] = from_f<T>(acc[q]);
        ov[i] = o;
      }
    } else {
      for (int i = lane; i < M; i += MOE_WAVE) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (live[j]) acc += sc[j] * to_f(er[j][i]);
        orow[i] = from_f<T>(acc);
      }
    }
  }
}

// one wave per (j, s); lanes stride over m, then a fixed-order butterfly
template <typename T, bool VEC>
__global__ void moe_row_dot_kernel(const T* __restrict__ g,
                                   const T* __restrict__ eo,
                                   const int* __restrict__ dest,
                                   float* __restrict__ gw, int k, int S,
                                   size_t R, int M) {
  constexpr int V = Vec16<T>::N;
  using VT = Vec16<T>;
  const int lane = threadIdx.x & (MOE_WAVE - 1);
  const size_t wave0 = (size_t)blockIdx.x * MOE_WAVES + threadIdx.x / MOE_WAVE;
  const size_t nwaves = (size_t)gridDim.x * MOE_WAVES;
  const size_t n = (size_t)k * S;
  for (size_t p = wave0; p < n; p += nwaves) {
    const size_t s = p % (size_t)S;
    const int d = dest[p];
    float acc = 0.f;
    if (d >= 0 && (size_t)d < R) {  // wave-uniform
      const T* gr = g + s * M;
      const T* er = eo + (size_t)d * M;
      if (VEC) {
        const int nv = M / V;
        const VT* gv = reinterpret_cast<const VT*>(gr);
        const VT* ev = reinterpret_cast<const VT*>(er);
        for (int i = lane; i < nv; i += MOE_WAVE) {
          const VT a = gv[i], b = ev[i];
#pragma unroll
          for (int q = 0; q < V; ++q) acc += to_f(a.v[q]) * to_f(b.v[q]);
        }
      } else {
        for (int i = lane; i < M; i += MOE_WAVE)
          acc += to_f(gr[i]) * to_f(er[i]);
      }
    }
#pragma unroll
    for (int off = MOE_WAVE / 2; off > 0; off >>= 1)
      acc += __shfl_xor(acc, off, MOE_WAVE);
    if (lane == 0) gw[p] = acc;
  }
}

inline unsigned row_grid(size_t rows) {
  size_t blocks = (rows + MOE_WAVES - 1) / MOE_WAVES;
  if (blocks > MOE_MAX_GRID) blocks = MOE_MAX_GRID;
  return (unsigned)(blocks ? blocks : 1);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <typename T>
void gather_rows_t(const void* x, const int* src, void* out, const float* w,
                   const int* dest, int k, int S, size_t R, int M,
                   hipStream_t stream) {
  const bool vec = ((size_t)M * sizeof(T)) % 16 == 0 && aligned16(x) &&
                   aligned16(out);
  const dim3 grid(row_grid(R)), block(MOE_BLOCK);
  if (vec)
    hipLaunchKernelGGL((moe_gather_rows_kernel<T, true>), grid, block, 0,
                       stream, (const T*)x, src, (T*)out, w, dest, k, S, R,
                       M);
  else
    hipLaunchKernelGGL((moe_gather_rows_kernel<T, false>), grid, block, 0,
                       stream, (const T*)x, src, (T*)out, w, dest, k, S, R,
                       M);
}

template <typename T, int K>
void combine_rows_tk(const void* eo, const int* dest, void* out,
                     const float* w, int S, size_t R, int M,
                     hipStream_t stream) {
  const bool vec = ((size_t)M * sizeof(T)) % 16 == 0 && aligned16(eo) &&
                   aligned16(out);
  const dim3 grid(row_grid((size_t)S)), block(MOE_BLOCK);
  if (vec)
    hipLaunchKernelGGL((moe_combine_rows_kernel<T, true, K>), grid, block, 0,
                       stream, (const T*)eo, dest, (T*)out, w, S, R, M);
  else
    hipLaunchKernelGGL((moe_combine_rows_kernel<T, false, K>), grid, block,
                       0, stream, (const T*)eo, dest, (T*)out, w, S, R, M);
}

template <typename T>
void row_dot_t(const void* g, const void* eo, const int* dest, float* gw,
               int k, int S, size_t R, int M, hipStream_t stream) {
  const bool vec = ((size_t)M * sizeof(T)) % 16 == 0 && aligned16(g) &&
                   aligned16(eo);
  const dim3 grid(row_grid((size_t)k * S)), block(MOE_BLOCK);
  if (vec)
    hipLaunchKernelGGL((moe_row_dot_kernel<T, true>), grid, block, 0, stream,
                       (const T*)g, (const T*)eo, dest, gw, k, S, R, M);
  else
    hipLaunchKernelGGL((moe_row_dot_kernel<T, false>), grid, block, 0,
                       stream, (const T*)g, (const T*)eo, dest, gw, k, S, R,
                       M);
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers (dtype: 0=f32 1=f16 2=bf16)
// ---------------------------------------------------------------------------

extern "C" {

// number of int32 the caller must provide as `hist` workspace
size_t bagua_moe_assign_workspace(int S, int E) {
  const size_t nblocks = ((size_t)S + MOE_BLOCK - 1) / MOE_BLOCK;
  return (nblocks ? nblocks : 1) * (size_t)E;
}

void bagua_moe_assign_slots_launch(const int* expert, int S, int E,
                                   int capacity, const int* base, int* hist,
                                   int* slot, int* counts, int* src,
                                   hipStream_t stream) {
  const int nblocks = (S + MOE_BLOCK - 1) / MOE_BLOCK;
  const size_t lds = (size_t)E * sizeof(int);
  if (nblocks > 0)
    hipLaunchKernelGGL(moe_hist_kernel, dim3(nblocks), dim3(MOE_BLOCK), lds,
                       stream, expert, S, E, hist);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(1024), 0, stream, hist,
                     nblocks, E, base, counts);
  if (nblocks > 0)
    hipLaunchKernelGGL(moe_rank_kernel, dim3(nblocks), dim3(MOE_BLOCK), lds,
                       stream, expert, S, E, capacity, hist, slot, src);
}

void bagua_moe_gather_rows_launch(int dtype, const void* x, const int* src,
                                  void* out, const float* w, const int* dest,
                                  int k, int S, size_t R, int M,
                                  hipStream_t stream) {
  if (R == 0 || M == 0) return;
  if (dtype == 0)
    gather_rows_t<float>(x, src, out, w, dest, k, S, R, M, stream);
  else if (dtype == 1)
    gather_rows_t<__half>(x, src, out, w, dest, k, S, R, M, stream);
  else
    gather_rows_t<__hip_bfloat16>(x, src, out, w, dest, k, S, R, M, stream);
}

void bagua_moe_combine_rows_launch(int dtype, const void* eo,
                                   const int* dest, void* out,
                                   const float* w, int k, int S, size_t R,
                                   int M, hipStream_t stream) {
  if (S == 0 || M == 0) return;
#define MOE_COMBINE(T)                                                     \
  do {                                                                     \
    if (k == 1)                                                            \
      combine_rows_tk<T, 1>(eo, dest, out, w, S, R, M, stream);            \
    else                                                                   \
      combine_rows_tk<T, 2>(eo, dest, out, w, S, R, M, stream);            \
  } while (0)
  if (dtype == 0)
    MOE_COMBINE(float);
  else if (dtype == 1)
    MOE_COMBINE(__half);
  else
    MOE_COMBINE(__hip_bfloat16);
#undef MOE_COMBINE
}

void bagua_moe_row_dot_launch(int dtype, const void* g, const void* eo,
                              const int* dest, float* gw, int k, int S,
                              size_t R, int M, hipStream_t stream) {
  if (S == 0) return;
  if (dtype == 0)
    row_dot_t<float>(g, eo, dest, gw, k, S, R, M, stream);
  else if (dtype == 1)
    row_dot_t<__half>(g, eo, dest, gw, k, S, R, M, stream);
  else
    row_dot_t<__hip_bfloat16>(g, eo, dest, gw, k, S, R, M, stream);
}

}  // extern "C"
