// CDNA4 (gfx950) kernels for the first stage of a VGG-style network:
// Conv2d(3, 64, 3, padding=1) -> ReLU on a channels-last bf16 image, forward
// and backward, each as one pass over the 64-channel activation.
//
//   forward    y = relu(bf16(bf16(acc) + b)), acc = f32 sum of the 27 products
//   backward   dx = y <= 0 ? 0 : g  (in registers and LDS only),
//              dW[co][k] = sum_pixels dx[pixel][co] * patch[pixel][k],
//              db[co]    = sum_pixels dx[pixel][co]
//
// The image needs no gradient, so dx is never written to memory. The two
// roundings of the forward are those of the unfused chain (the convolution
// rounds to bf16, the in-place bias add rounds again); NaN and -0.0 go
// through bias + ReLU as in epilogue_kernels.hip.
//
// Both kernels are implicit GEMMs on __builtin_amdgcn_mfma_f32_32x32x16_bf16
// with the patch index k = (ky*3 + kx)*3 + ci, 27 padded to 32. A 256-thread
// block works on tiles of FC_TH x FC_TW output pixels of one image, wave w
// on row w of the tile. The input tile with its one-pixel halo (about 1.2 KB)
// is staged in LDS; halo pixels outside the image are zero and a tile never
// reads across a row or image boundary. The next tile's global loads are
// issued into registers before the current tile's MFMAs.
//
//   forward    D[channel][pixel] = W[channel][k] . patch[k][pixel]. The MFMA
//              rows are a permutation of the channels (bits 2 and 3 swapped)
//              such that a lane ends up with 8 consecutive channels of its
//              pixel in 8 consecutive registers. The rounded tile goes
//              through LDS once, so that the global stores are 16-byte
//              vectors with consecutive lanes on consecutive addresses.
//   backward   D[channel][k] = dx^T[channel][pixel] . patch[pixel][k], summed
//              over the pixel index; column 27 of the patch operand is 1.0,
//              which yields db from the same MFMAs. g and y come in with
//              16-byte loads, the masked dx tile is transposed through LDS.
//              A block keeps its f32 accumulators over a fixed contiguous
//              range of tiles and writes one [64 x 28] partial; a finalize
//              kernel sums the partials in a fixed order, rounds once to
//              bf16 and writes dW through the weight's strides. No atomics:
//              two runs give the same bits.

#include <hip/hip_runtime.h>
#include <cstdint>

#define FC_BLOCK 256
#define FC_WAVES (FC_BLOCK / 64)
#define FC_TW 32                        // tile width: the MFMA's 32 columns
#define FC_TH FC_WAVES                  // tile height: one row per wave
#define FC_CIN 3
#define FC_COUT 64
#define FC_K 27
#define FC_KB 28                        // patch columns + the column of ones
#define FC_XROW ((FC_TW + 2) * FC_CIN)  // bf16 elements of a halo row
#define FC_XTILE ((FC_TH + 2) * FC_XROW)
#define FC_XLOADS ((FC_XTILE + FC_BLOCK - 1) / FC_BLOCK)
#define FC_VEC_PER_ROW (FC_TW * FC_COUT / 8)  // 16-byte vectors of a tile row
// finalize: 8 outputs x 32 slices of the partial rows per block
#define FC_FIN_OUT 8
#define FC_FIN_SL (FC_BLOCK / FC_FIN_OUT)

static_assert(FC_VEC_PER_ROW == FC_BLOCK, "one 16-byte vector per thread and "
                                          "tile row");
static_assert((FC_COUT * FC_KB) % FC_FIN_OUT == 0, "finalize grid");

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

union Frag {
  bf16x8 v;
  uint16_t e[8];
  uint4 q;
};

__device__ __forceinline__ float bf16_to_f(uint16_t b) {
  return __uint_as_float((uint32_t)b << 16);
}

// torch's rounding (c10 round_to_nearest_even), NaN payload included
__device__ __forceinline__ uint16_t f_to_bf16(float v) {
  if (v != v) return 0x7FC0;
  const uint32_t u = __float_as_uint(v);
  return (uint16_t)((u + ((u >> 16) & 1u) + 0x7FFFu) >> 16);
}

// relu(bf16(x + b)) as add_ then clamp_min_(0) give it
__device__ __forceinline__ uint16_t bias_relu(uint16_t x, float b) {
  const uint16_t t = f_to_bf16(bf16_to_f(x) + b);
  const float f = bf16_to_f(t);
  // fmaxf(f, 0) is f or a zero, both exact in bf16: its high half is it
  return (f != f) ? t : (uint16_t)(__float_as_uint(fmaxf(f, 0.f)) >> 16);
}

struct Geom {
  int H, W, tiles_x, tiles_y, ntiles;
};

struct TilePos {
  int n, y0, x0;
};

__device__ __forceinline__ TilePos tile_pos(int t, const Geom& g) {
  TilePos p;
  const int tx = t % g.tiles_x;
  const int q = t / g.tiles_x;
  const int ty = q % g.tiles_y;
  p.n = q / g.tiles_y;
  p.y0 = ty * FC_TH;
  p.x0 = tx * FC_TW;
  return p;
}

// The thread's share of the input tile with halo, global -> registers.
// Element e of the tile is (row e / FC_XROW, then pixel and channel); a row
// is contiguous in memory. Outside the image: zero.
__device__ __forceinline__ void load_x_tile(const uint16_t* __restrict__ x,
                                            const Geom& g, const TilePos& p,
                                            uint16_t (&xr)[FC_XLOADS]) {
#pragma unroll
  for (int u = 0; u < FC_XLOADS; ++u) {
    const int e = (int)threadIdx.x + u * FC_BLOCK;
    xr[u] = 0;
    if (e < FC_XTILE) {
      const int ty = e / FC_XROW;
      const int rem = e - ty * FC_XROW;
      const int tx = rem / FC_CIN;
      const int gy = p.y0 - 1 + ty, gx = p.x0 - 1 + tx;
      if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
        const size_t pix = ((size_t)p.n * g.H + gy) * g.W + gx;
        xr[u] = x[pix * FC_CIN + (rem - tx * FC_CIN)];
      }
    }
  }
}

__device__ __forceinline__ void store_x_tile(uint16_t* xt,
                                             const uint16_t (&xr)[FC_XLOADS]) {
#pragma unroll
  for (int u = 0; u < FC_XLOADS; ++u) {
    const int e = (int)threadIdx.x + u * FC_BLOCK;
    if (e < FC_XTILE) xt[e] = xr[u];
  }
}

// offset of patch element k (< 27) from a pixel's top-left halo element
__device__ __forceinline__ int patch_off(int k) {
  const int ky = k / 9;
  return ky * FC_XROW + (k - ky * 9);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(FC_BLOCK)
first_conv_fwd_kernel(const uint16_t* __restrict__ x,
                      const uint16_t* __restrict__ w, long ws0, long ws1,
                      long ws2, long ws3, const uint16_t* __restrict__ bias,
                      uint4* __restrict__ y, Geom g) {
  __shared__ uint16_t xt[FC_XTILE];
  __shared__ uint4 yt[FC_TH * FC_VEC_PER_ROW];  // the rounded output tile

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;

  // A operand: row r of M-tile mt is channel 32*mt + (r with bits 2 and 3
  // swapped); then registers 8*gh .. 8*gh+7 of a lane's accumulator are the
  // channels 32*mt + 16*gh + 8*h + 0..7 of its pixel
  const int rc = (r & 0x13) | ((r & 4) << 1) | ((r & 8) >> 1);
  Frag a[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * s + 8 * h + j;
      const bool in = k < FC_K;
      const int ky = k / 9, kx = (k / 3) % 3, ci = k % 3;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const long co = 32 * mt + rc;
        a[mt][s].e[j] =
            in ? w[co * ws0 + ci * ws1 + ky * ws2 + kx * ws3] : (uint16_t)0;
      }
    }
  }
  // element loads: a bias that is a view into a flat parameter buffer need
  // not be 16-byte aligned
  Frag b[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      b[t].e[q] = bias[32 * (t >> 1) + 16 * (t & 1) + 8 * h + q];
  }

  uint16_t xr[FC_XLOADS];
  int t = blockIdx.x;
  if (t < g.ntiles) load_x_tile(x, g, tile_pos(t, g), xr);
  for (; t < g.ntiles; t += gridDim.x) {
    const TilePos p = tile_pos(t, g);
    __syncthreads();  // the previous tile's reads of xt and yt are done
    store_x_tile(xt, xr);
    __syncthreads();
    if (t + (int)gridDim.x < g.ntiles)
      load_x_tile(x, g, tile_pos(t + gridDim.x, g), xr);

    // B operand: column r is pixel (wave, r) of the tile
    const uint16_t* px = xt + wave * FC_XROW + r * FC_CIN;
    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Frag bf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // k = 16 * s + 8 * h + j; lane half 1 of the second step runs out
        // of patch elements at j = 3
        const int k0 = 16 * s + j, k1 = k0 + 8;
        const int off = h ? (k1 < FC_K ? patch_off(k1) : 0) : patch_off(k0);
        const uint16_t v = px[off];
        bf.e[j] = (k1 < FC_K || !h) ? v : (uint16_t)0;
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt][s].v, bf.v,
                                                          acc[mt], 0, 0, 0);
    }

    // round, bias, ReLU; 16-byte chunk c of pixel r goes to slot c ^ (r & 7)
    // of the pixel's 128-byte row so that the 64 lanes spread over the banks
    uint4* yw = yt + wave * FC_VEC_PER_ROW;
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) {
      Frag o;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        o.e[q] = bias_relu(f_to_bf16(acc[tq >> 1][8 * (tq & 1) + q]),
                           bf16_to_f(b[tq].e[q]));
      const int chunk = 4 * (tq >> 1) + 2 * (tq & 1) + h;
      yw[r * 8 + (chunk ^ (r & 7))] = o.q;
    }
    __syncthreads();
    const int gy = p.y0 + wave;
    if (gy < g.H) {
      uint4* yrow = y + (((size_t)p.n * g.H + gy) * g.W + p.x0) * (FC_COUT / 8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = i * 64 + lane;  // vector of the row, in memory order
        const int pr = v >> 3, chunk = v & 7;
        if (p.x0 + pr < g.W) yrow[v] = yw[pr * 8 + (chunk ^ (pr & 7))];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// One tile row per u: the thread's vector is pixel threadIdx.x / 8, channels
// 8 * (threadIdx.x % 8) .. + 7. Outside the image g and y are zero, which
// makes dx zero there.
__device__ __forceinline__ void load_gy_tile(const uint4* __restrict__ gv,
                                             const uint4* __restrict__ yv,
                                             const Geom& g, const TilePos& p,
                                             uint4 (&gr)[FC_TH],
                                             uint4 (&yr)[FC_TH]) {
  const int pr = threadIdx.x >> 3;
#pragma unroll
  for (int u = 0; u < FC_TH; ++u) {
    gr[u] = make_uint4(0, 0, 0, 0);
    yr[u] = make_uint4(0, 0, 0, 0);
    const int gy = p.y0 + u;
    if (gy < g.H && p.x0 + pr < g.W) {
      const size_t v = (((size_t)p.n * g.H + gy) * g.W + p.x0) * (FC_COUT / 8)
                       + threadIdx.x;
      gr[u] = gv[v];
      yr[u] = yv[v];
    }
  }
}

// two bf16 in a word: g where !(y <= 0), else +0.0 (threshold_backward)
__device__ __forceinline__ uint32_t relu_mask2(uint32_t g, uint32_t y) {
  const float ylo = __uint_as_float(y << 16);
  const float yhi = __uint_as_float(y & 0xFFFF0000u);
  uint32_t m = 0xFFFFFFFFu;
  if (ylo <= 0.f) m &= 0xFFFF0000u;
  if (yhi <= 0.f) m &= 0x0000FFFFu;
  return g & m;
}

__global__ void __launch_bounds__(FC_BLOCK)
first_conv_bwd_kernel(const uint4* __restrict__ gv,
                      const uint4* __restrict__ yv,
                      const uint16_t* __restrict__ x,
                      float* __restrict__ partial, Geom g) {
  __shared__ uint16_t xt[FC_XTILE];
  // dx of the tile as [pixel][channel]; afterwards the block's f32 sums
  __shared__ uint4 dxt[FC_TH * FC_VEC_PER_ROW];
  static_assert(sizeof(dxt) >= 2 * 16 * 64 * sizeof(float), "reduce buffer");

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;

  // this block's tiles: a fixed contiguous range, all ranges within one tile
  // of the same length
  const int lo = (int)((long)blockIdx.x * g.ntiles / gridDim.x);
  const int hi = (int)((long)(blockIdx.x + 1) * g.ntiles / gridDim.x);

  // B operand: column r is patch element r, column 27 is 1.0, the rest 0
  const int coff = r < FC_K ? patch_off(r) : 0;
  const uint16_t bconst = r == FC_K ? (uint16_t)0x3F80 : (uint16_t)0;

  f32x16 acc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
  }

  uint4 gr[FC_TH], yr[FC_TH];
  uint16_t xr[FC_XLOADS];
  if (lo < hi) {
    const TilePos p = tile_pos(lo, g);
    load_gy_tile(gv, yv, g, p, gr, yr);
    load_x_tile(x, g, p, xr);
  }
  for (int t = lo; t < hi; ++t) {
    const TilePos pc = tile_pos(t, g);
    // pixels of this wave's tile row that lie in the image: beyond them dx
    // is zero, and so must the patch be, or a NaN or Inf at the image's
    // edge would reach taps that never see it (0 * NaN)
    const int wlim = pc.y0 + wave < g.H ? g.W - pc.x0 : 0;
    __syncthreads();  // the previous tile's reads of xt and dxt are done
#pragma unroll
    for (int u = 0; u < FC_TH; ++u) {
      uint4 d;
      d.x = relu_mask2(gr[u].x, yr[u].x);
      d.y = relu_mask2(gr[u].y, yr[u].y);
      d.z = relu_mask2(gr[u].z, yr[u].z);
      d.w = relu_mask2(gr[u].w, yr[u].w);
      dxt[u * FC_VEC_PER_ROW + threadIdx.x] = d;
    }
    store_x_tile(xt, xr);
    __syncthreads();
    if (t + 1 < hi) {
      const TilePos p = tile_pos(t + 1, g);
      load_gy_tile(gv, yv, g, p, gr, yr);
      load_x_tile(x, g, p, xr);
    }

    // wave w sums over the 32 pixels of tile row w, 16 per MFMA
    const uint16_t* dxe = reinterpret_cast<const uint16_t*>(dxt) +
                          wave * FC_TW * FC_COUT;
    const uint16_t* px = xt + wave * FC_XROW + coff;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      Frag bf, af[2];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int pix = 16 * ks + 8 * h + j;
        const uint16_t bv = r < FC_K ? px[pix * FC_CIN] : bconst;
        bf.e[j] = pix < wlim ? bv : (uint16_t)0;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
          af[mt].e[j] = dxe[pix * FC_COUT + 32 * mt + r];
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt].v, bf.v,
                                                          acc[mt], 0, 0, 0);
    }
  }

  // waves 0..3 add their sums in that order, then the block's partial goes
  // out as [channel][FC_KB]
  float* red = reinterpret_cast<float*>(dxt);
  for (int wv = 0; wv < FC_WAVES; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int idx = (mt * 16 + i) * 64 + lane;
          red[idx] = wv == 0 ? acc[mt][i] : red[idx] + acc[mt][i];
        }
      }
    }
  }
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * (FC_COUT * FC_KB);
  for (int idx = threadIdx.x; idx < 2 * 16 * 64; idx += FC_BLOCK) {
    const int mt = idx >> 10, i = (idx >> 6) & 15, ln = idx & 63;
    const int col = ln & 31;
    const int row = (i & 3) + 8 * (i >> 2) + 4 * (ln >> 5);
    if (col < FC_KB) out[(32 * mt + row) * FC_KB + col] = red[idx];
  }
}

// dW[co][k] and db[co] = bf16(sum over the partial rows, in a fixed order);
// dW is written through the weight's strides (co, ci, ky, kx)
__global__ void __launch_bounds__(FC_BLOCK)
first_conv_bwd_finalize_kernel(const float* __restrict__ partial, int nrows,
                               uint16_t* __restrict__ dw, long ws0, long ws1,
                               long ws2, long ws3, uint16_t* __restrict__ db) {
  __shared__ float red[FC_FIN_SL][FC_FIN_OUT];
  const int cl = threadIdx.x % FC_FIN_OUT, sl = threadIdx.x / FC_FIN_OUT;
  const int o = blockIdx.x * FC_FIN_OUT + cl;  // < FC_COUT * FC_KB
  float s = 0.f;
#pragma unroll 8
  for (int b = sl; b < nrows; b += FC_FIN_SL)
    s += partial[(size_t)b * (FC_COUT * FC_KB) + o];
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < FC_FIN_SL; ++k) t += red[k][cl];
    const long co = o / FC_KB;
    const int k = o - (int)co * FC_KB;
    if (k == FC_K) {
      db[co] = f_to_bf16(t);
    } else {
      const int ky = k / 9, kx = (k / 3) % 3, ci = k % 3;
      dw[co * ws0 + ci * ws1 + ky * ws2 + kx * ws3] = f_to_bf16(t);
    }
  }
}

inline Geom geom_of(int N, int H, int W) {
  Geom g;
  g.H = H;
  g.W = W;
  g.tiles_x = (W + FC_TW - 1) / FC_TW;
  g.tiles_y = (H + FC_TH - 1) / FC_TH;
  // every tile holds a pixel and N*H*W < 2^31, so this fits
  g.ntiles = N * g.tiles_y * g.tiles_x;
  return g;
}

// Grid caps, fixed as in epilogue_kernels.hip: the blocks 256 CUs hold at
// once at the kernels' register counts (forward two, backward three 4-wave
// blocks per CU). With fewer blocks resident the rest queue behind them.
#define FC_FWD_MAX_GRID 512
// The backward's blocks own contiguous tile ranges, so its cap should not
// exceed what is resident; it also keeps the f32 partials at 5.5 MB.
#define FC_BWD_MAX_GRID 768

inline unsigned grid_of(const Geom& g, int cap) {
  return (unsigned)(g.ntiles < cap ? g.ntiles : cap);
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers. The caller has checked: bf16, x (N, 3, H, W) and g, y
// (N, 64, H, W) channels-last contiguous, g and y 16-byte aligned,
// 1 <= N*H*W < 2^31, the weight's (co, ci, ky, kx) strides address 64*27
// distinct elements.
// ---------------------------------------------------------------------------

extern "C" {

// rows of the f32 partial buffer [blocks, 64 * 28] the backward needs
size_t bagua_first_conv_partial_rows(int N, int H, int W) {
  return grid_of(geom_of(N, H, W), FC_BWD_MAX_GRID);
}

size_t bagua_first_conv_partial_cols() { return FC_COUT * FC_KB; }

void bagua_first_conv_fwd_launch(const void* x, const void* w,
                                 const long* wstride, const void* bias,
                                 void* y, int N, int H, int W,
                                 hipStream_t stream) {
  const Geom g = geom_of(N, H, W);
  hipLaunchKernelGGL(first_conv_fwd_kernel, dim3(grid_of(g, FC_FWD_MAX_GRID)), dim3(FC_BLOCK), 0,
                     stream, (const uint16_t*)x, (const uint16_t*)w,
                     wstride[0], wstride[1], wstride[2], wstride[3],
                     (const uint16_t*)bias, (uint4*)y, g);
}

void bagua_first_conv_bwd_launch(const void* g, const void* y, const void* x,
                                 float* partial, void* dw,
                                 const long* wstride, void* db, int N, int H,
                                 int W, hipStream_t stream) {
  const Geom gm = geom_of(N, H, W);
  const unsigned grid = grid_of(gm, FC_BWD_MAX_GRID);
  hipLaunchKernelGGL(first_conv_bwd_kernel, dim3(grid), dim3(FC_BLOCK), 0,
                     stream, (const uint4*)g, (const uint4*)y,
                     (const uint16_t*)x, partial, gm);
  hipLaunchKernelGGL(first_conv_bwd_finalize_kernel,
                     dim3(FC_COUT * FC_KB / FC_FIN_OUT), dim3(FC_BLOCK), 0,
                     stream, (const float*)partial, (int)grid,
                     (uint16_t*)dw, wstride[0], wstride[1], wstride[2],
                     wstride[3], (uint16_t*)db);
}

}  // extern "C"
