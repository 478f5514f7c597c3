// The host-callable surface of the HIP sources: every launcher and sizing
// helper that core.cpp's bindings call, declared once. Each .hip file
// includes this header, so a definition that disagrees with its declaration
// does not compile (with C linkage the linker would match on the name
// alone). Plain C++, no device code. Nothing here synchronizes: a launcher
// enqueues on `stream` and returns.

#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

// The dtype code of every `int dtype` below (kernel_dtype() in core.cpp
// makes it from a tensor and throws for any other type).
enum BaguaDtype { BAGUA_F32 = 0, BAGUA_F16 = 1, BAGUA_BF16 = 2 };

extern "C" {

// ---------------------------------------------------------------------------
// kernels.hip
// ---------------------------------------------------------------------------

// x = op(x, y, f); op is an EwOp of kernels.hip (average, add, sub, addmul,
// div with f = 1 / divisor)
void bagua_ew_launch(int op, int dtype, void* x, const void* y, float f,
                     size_t n, hipStream_t stream);
// x += reduced / nranks - x_copy
void bagua_async_avg_launch(int dtype, void* x, const void* reduced,
                            const void* x_copy, float nranks, size_t n,
                            hipStream_t stream);
// x[target_chunk] = sum (or mean) over the num_chunks chunks of x
void bagua_reduce_chunk_launch(int dtype, void* x, int num_chunks,
                               int target_chunk, int average, size_t chunk,
                               hipStream_t stream);
// scratch: uint32[2*num_chunks_total]; out: chunked wire buffer
void bagua_compress_launch(int dtype, const void* x, uint8_t* out,
                           uint32_t* scratch, uint32_t* partials,
                           size_t chunk, size_t chunk_stride,
                           int num_chunks_total, int chunk_begin,
                           int chunk_count, hipStream_t stream);
void bagua_decompress_launch(int dtype, const uint8_t* in, void* x,
                             size_t chunk, size_t chunk_stride,
                             int chunk_begin, int chunk_count,
                             hipStream_t stream);
// fused dequantize + reduce of all wire chunks into the target chunk of the
// bucket that x is the base of; at most 64 chunks
void bagua_dequant_reduce_launch(int dtype, const uint8_t* in, void* x,
                                 size_t chunk, size_t chunk_stride,
                                 int num_chunks, int target_chunk,
                                 int average, hipStream_t stream);

// Fused optimizer steps, torch semantics. 1 - beta and the bias corrections
// bc1, bc2 come from the host, formed in double and cast once.
void bagua_fused_sgd_launch(float* p, const float* g, float* m, float lr,
                            float momentum, float dampening,
                            float weight_decay, int nesterov,
                            int momentum_initialized, size_t n,
                            hipStream_t stream);
void bagua_fused_adam_launch(float* p, const float* g, float* m, float* v,
                             float lr, float beta1, float beta2,
                             float one_minus_beta1, float one_minus_beta2,
                             float eps, float weight_decay, int adamw,
                             float bc1, float bc2, size_t n,
                             hipStream_t stream);
// p and g bf16, master and m f32
void bagua_fused_sgd_mixed_launch(void* p, const void* g, float* master,
                                  float* m, float lr, float momentum,
                                  float dampening, float weight_decay,
                                  int nesterov, int momentum_initialized,
                                  size_t n, hipStream_t stream);

// The segmented steps read the gradient where it lives. Segment k covers
// flat elements [begins[k], begins[k] + numels[k]); the segments are
// non-empty, ascending and contiguous (the caller checks). A null grads[k]
// is a zero gradient.
void bagua_fused_sgd_segments_launch(float* p, float* m, float lr,
                                     float momentum, float dampening,
                                     float weight_decay, int nesterov,
                                     int momentum_initialized,
                                     const void* const* grads,
                                     const size_t* begins,
                                     const size_t* numels, size_t count,
                                     hipStream_t stream);
void bagua_fused_sgd_mixed_segments_launch(
    void* p, float* master, float* m, float lr, float momentum,
    float dampening, float weight_decay, int nesterov,
    int momentum_initialized, const void* const* grads, const size_t* begins,
    const size_t* numels, size_t count, hipStream_t stream);
void bagua_fused_adam_segments_launch(
    float* p, float* m, float* v, float lr, float beta1, float beta2,
    float one_minus_beta1, float one_minus_beta2, float eps,
    float weight_decay, int adamw, float bc1, float bc2,
    const void* const* grads, const size_t* begins, const size_t* numels,
    size_t count, hipStream_t stream);

// how many segments (padding included) the momentum launcher can take
size_t bagua_qadam_momentum_max_segments();
// m: the bucket's flat f32 momentum, num_chunks * chunk elements; segment k
// covers [begins[k], begins[k] + numels[k]) from 0 on, what lies behind the
// last one is padding (zero gradient). out == nullptr: update only.
// Otherwise the update and then the wire of all chunks, as
// bagua_compress_launch(0, m, out, ..., 0, num_chunks) writes it.
void bagua_qadam_momentum_compress_launch(
    float* m, const void* const* grads, const size_t* begins,
    const size_t* numels, size_t count, float beta1, float one_minus_beta1,
    uint8_t* out, uint32_t* scratch, uint32_t* partials, size_t chunk,
    size_t chunk_stride, int num_chunks, hipStream_t stream);
// w, v flat; segment k of the momentum covers flat elements
// [begins[k], begins[k] + numels[k]), as the gradient does in the steps
// above
void bagua_qadam_frozen_segments_launch(
    float* p, const float* v, float lr, float eps, float bc1, float bc2,
    const void* const* moms, const size_t* begins, const size_t* numels,
    size_t count, hipStream_t stream);

// Cross-GPU flag barrier of the p2p alltoall: writes seq into slot `rank` of
// every peer's flag array, then waits until all nranks (<= 64) slots of
// my_flags have reached it.
void bagua_p2p_barrier_launch(void* peer_flags_dev_array, void* my_flags,
                              int rank, int nranks, unsigned long long seq,
                              hipStream_t stream);

// ---------------------------------------------------------------------------
// moe_kernels.hip
// ---------------------------------------------------------------------------

// number of int32 the caller must provide as `hist` workspace
size_t bagua_moe_assign_workspace(int S, int E);
void bagua_moe_assign_slots_launch(const int* expert, int S, int E,
                                   int capacity, const int* base, int* hist,
                                   int* slot, int* counts, int* src,
                                   hipStream_t stream);
void bagua_moe_gather_rows_launch(int dtype, const void* x, const int* src,
                                  void* out, const float* w, const int* dest,
                                  int k, int S, size_t R, int M,
                                  hipStream_t stream);
void bagua_moe_combine_rows_launch(int dtype, const void* eo,
                                   const int* dest, void* out,
                                   const float* w, int k, int S, size_t R,
                                   int M, hipStream_t stream);
void bagua_moe_row_dot_launch(int dtype, const void* g, const void* eo,
                              const int* dest, float* gw, int k, int S,
                              size_t R, int M, hipStream_t stream);

// ---------------------------------------------------------------------------
// epilogue_kernels.hip. The caller has checked: C is a multiple of the
// 16-byte vector and C / vector <= 256, full-size rows are below 2^31, data
// pointers are 16-byte aligned, H and W are even when pooling. `rows` counts
// full-size rows, `orows` pooled ones.
// ---------------------------------------------------------------------------

// rows of the f32 partial buffer [blocks, C] the backward launchers need;
// work_rows is `rows` without pooling and `orows` with it
size_t bagua_epi_partial_rows(int dtype, size_t work_rows, int C);
void bagua_epi_bias_relu_launch(int dtype, void* x, const void* bias,
                                size_t rows, int C, hipStream_t stream);
void bagua_epi_bias_relu_pool_launch(int dtype, void* x, const void* bias,
                                     void* p, size_t orows, int Wo, int C,
                                     hipStream_t stream);
// partial == nullptr: dx only, db is left alone
void bagua_epi_relu_bwd_launch(int dtype, const void* g, const void* y,
                               void* dx, float* partial, void* db,
                               size_t rows, int C, hipStream_t stream);
void bagua_epi_pool_relu_bwd_launch(int dtype, const void* g, const void* y,
                                    void* dx, float* partial, void* db,
                                    size_t orows, int Wo, int C,
                                    hipStream_t stream);
// The compact pair: x is only read; code is [orows, C] bytes, written by the
// forward for the backward alone, which then needs no y. dx and db are those
// of the pair above, bit for bit.
void bagua_epi_bias_relu_pool_code_launch(int dtype, const void* x,
                                          const void* bias, void* p,
                                          uint8_t* code, size_t orows, int Wo,
                                          int C, hipStream_t stream);
void bagua_epi_pool_code_bwd_launch(int dtype, const void* g,
                                    const uint8_t* code, void* dx,
                                    float* partial, void* db, size_t orows,
                                    int Wo, int C, hipStream_t stream);

// ---------------------------------------------------------------------------
// first_conv_kernels.hip. The caller has checked: bf16, x (N, 3, H, W) and
// g, y (N, 64, H, W) channels-last contiguous, g and y 16-byte aligned,
// 1 <= N*H*W < 2^31, the weight's (co, ci, ky, kx) strides address 64*27
// distinct elements.
// ---------------------------------------------------------------------------

// rows and columns of the f32 partial buffer the backward needs
size_t bagua_first_conv_partial_rows(int N, int H, int W);
size_t bagua_first_conv_partial_cols();
void bagua_first_conv_fwd_launch(const void* x, const void* w,
                                 const long* wstride, const void* bias,
                                 void* y, int N, int H, int W,
                                 hipStream_t stream);
void bagua_first_conv_bwd_launch(const void* g, const void* y, const void* x,
                                 float* partial, void* dw,
                                 const long* wstride, void* db, int N, int H,
                                 int W, hipStream_t stream);

// ---------------------------------------------------------------------------
// batchnorm_kernels.hip. layout: 0 rows [N, C], 1 planes [N, C, S] element
// by element, 2 planes in 16-byte vectors. The caller has checked: N * C * S
// is positive and below 2^31; with layout 0, C is a multiple of the 16-byte
// vector, S is 1 (N counts rows) and the data pointers are 16-byte aligned;
// with layout 2, S * sizeof(T) is a multiple of 16 and the data pointers are
// aligned. *_f32 say whether a per-channel vector is f32 (else it has the
// data's dtype).
// ---------------------------------------------------------------------------

// rows of the f32 partial buffer [rows, 2C] that the reducing launchers need
size_t bagua_bn_partial_rows(int dtype, int layout, size_t N, int C,
                             size_t S);
// stats = (sum x [C], sum x*x [C], N*S)
void bagua_bn_stats_launch(int dtype, int layout, const void* x,
                           float* partial, float* stats, size_t N, int C,
                           size_t S, hipStream_t stream);
// w, b and rmean/rvar may be null. act: 0 none, 1 y = relu(bn(x)),
// 2 y = relu(bn(x) + z). z (act 2 only, else null) is laid out and aligned
// as x. mask (act 1 and 2 with layout 0 only, else null) receives
// [N, C / vector] bytes, bit k of a byte set where element k of that
// 16-byte vector of y is above zero.
void bagua_bn_apply_launch(int dtype, int layout, int act, const void* x,
                           const void* z, void* y, void* mask,
                           const float* stats, float* mean_invstd,
                           const void* w, int w_f32, const void* b, int b_f32,
                           void* rmean, void* rvar, int r_f32, float momentum,
                           float one_minus_momentum, float eps, size_t N,
                           int C, size_t S, hipStream_t stream);
// packed = (sum dy [C], sum dy*(x-mean) [C]); gw and gb may be null.
// saved: null, or what a forward with act 1 or 2 left, its mask with layout
// 0 and its y (laid out and aligned as x) otherwise; dy then counts only
// where that y is above zero.
void bagua_bn_bwd_reduce_launch(int dtype, int layout, const void* dy,
                                const void* x, const void* saved,
                                const float* mean_invstd, float* partial,
                                float* packed, void* gw, int gw_f32, void* gb,
                                int gb_f32, size_t N, int C, size_t S,
                                hipStream_t stream);
// w may be null. saved as above; dz (null without saved, and may be null
// with it) receives the masked dy, laid out and aligned as x.
void bagua_bn_bwd_apply_launch(int dtype, int layout, const void* dy,
                               const void* x, const void* saved, void* dx,
                               void* dz, const float* packed,
                               const float* stats, const float* mean_invstd,
                               const void* w, int w_f32, size_t N, int C,
                               size_t S, hipStream_t stream);

// ---------------------------------------------------------------------------
// layernorm_kernels.hip. Rows [R, H], normalised over H:
//   s = x + keep * (h + bias) * scale,  y = (s - mean) * rstd * gamma + beta
// x, s, y, dy and dx have the dtype x_dtype; h and dh have h_dtype, which is
// x_dtype, or f16/bf16 under an f32 x. The caller has checked: H % 8 == 0,
// 8 <= H <= BAGUA_LN_HMAX, 0 < R * H < 2^31, rows contiguous, every data
// pointer (x, h, y, s, dy, dx, dh) 16-byte aligned, mask [R, H / 8] bytes,
// mean and rstd [R] f32. *_f32 say whether a per-column vector is f32; else
// bias and dbias have h_dtype, gamma, beta and their gradients x_dtype.
// ---------------------------------------------------------------------------

// longest row, waves (rows in flight) of a block, and the cap on the blocks
// of the forward kernel, which grid-strides over rows
#define BAGUA_LN_HMAX 4096
#define BAGUA_LN_WAVES 4
#define BAGUA_LN_FWD_MAX_GRID 2048

// h, bias, gamma, beta may be null; h null is plain LayerNorm of x, and then
// s may be null (it would be x). Dropout happens where mask is not null:
// seed is one 64-bit word in device memory, an element is kept where its
// 32 random bits are at or above drop_threshold = p * 2^32, scale is
// 1 / (1 - p), and mask receives bit k of byte j of a row for element
// 8 * j + k. Without mask, scale is 1.
void bagua_ln_fwd_launch(int x_dtype, int h_dtype, const void* x,
                         const void* h, const void* bias, int bias_f32,
                         const void* gamma, int gamma_f32, const void* beta,
                         int beta_f32, const int64_t* seed,
                         uint32_t drop_threshold, float scale, void* y,
                         void* s, float* mean, float* rstd, uint8_t* mask,
                         float eps, size_t R, int H, hipStream_t stream);
// rows of the f32 partial buffer [rows, 3H] that the backward needs when a
// column sum is wanted
size_t bagua_ln_partial_rows(size_t R);
// dx = ds. With a branch (has_branch), dh = ds * keep * scale where mask is
// given and ds otherwise; a null dh is not written (the caller uses dx).
// dgamma, dbeta and dbias are written where not null, dbias only with a
// branch; partial may be null when all three are.
void bagua_ln_bwd_launch(int x_dtype, int h_dtype, const void* dy,
                         const void* s, const float* mean, const float* rstd,
                         const void* gamma, int gamma_f32,
                         const uint8_t* mask, float scale, int has_branch,
                         void* dx, void* dh, float* partial, void* dgamma,
                         int dgamma_f32, void* dbeta, int dbeta_f32,
                         void* dbias, int dbias_f32, size_t R, int H,
                         hipStream_t stream);

// ---------------------------------------------------------------------------
// bias_gelu_kernels.hip. Rows [R, C]:
//   z = h + bias,  a = gelu(z);  dh = dy * gelu'(z),  db = column sums of dh
// in the erf form, or with tanh_form the tanh form. h, a, dy and dh have the
// dtype `dtype`. The caller has checked: C % 8 == 0, C >= 8 (no upper
// limit), 0 < R * C < 2^31, rows contiguous, every data pointer 16-byte
// aligned. bias may be null (plain GELU); bias_f32 and db_f32 say whether
// the vector is f32, else it has the data's dtype.
// ---------------------------------------------------------------------------

// threads of a block; chunks (8 elements) of a row in a column tile, one
// tile per blockIdx.x; the cap on the blocks of a grid, which grid-strides
// over rows; and the bound on the backward's f32 partial buffer, which a
// single row of more than BAGUA_BG_PARTIAL_BYTES / 4 columns exceeds (it is
// then that one row)
#define BAGUA_BG_BLOCK 256
#define BAGUA_BG_TILE_CHUNKS 64
#define BAGUA_BG_MAX_GRID 1024
#define BAGUA_BG_PARTIAL_BYTES (2u << 20)

void bagua_bias_gelu_fwd_launch(int dtype, int tanh_form, const void* h,
                                const void* bias, int bias_f32, void* a,
                                size_t R, int C, hipStream_t stream);
// rows of the f32 partial buffer [rows, C] that the backward needs for db
size_t bagua_bias_gelu_partial_rows(size_t R, int C);
// db is written where db, bias and partial are all given; without a bias
// there is nothing to sum
void bagua_bias_gelu_bwd_launch(int dtype, int tanh_form, const void* dy,
                                const void* h, const void* bias, int bias_f32,
                                void* dh, float* partial, void* db,
                                int db_f32, size_t R, int C,
                                hipStream_t stream);

// ---------------------------------------------------------------------------
// attention_kernels.hip. Self-attention over a packed qkv (B, S, 3H), last
// dimension (3, heads, BAGUA_ATT_HEAD_DIM), with a length per sequence:
// rows at or behind clamp(seq_lens[b], 0, S) are not attended, are never
// loaded, and come out as zeros in out (B, S, H) and dqkv (B, S, 3H).
// seq_lens may be null (every length is S). lse and delta are
// (B, heads, S) f32. The caller has checked: f16 or bf16, everything
// contiguous, qkv, out, dout and dqkv 16-byte aligned, B, S, heads >= 1,
// B and heads <= 65535, B * S * 3H < 2^31.
// ---------------------------------------------------------------------------

// queries a forward block takes and keys it stages at a time; backward uses
// the same two numbers (its key blocks take BLOCK_M keys and stage BLOCK_N
// queries)
#define BAGUA_ATT_BLOCK_M 128
#define BAGUA_ATT_BLOCK_N 64
#define BAGUA_ATT_HEAD_DIM 64

void bagua_attention_fwd_launch(int dtype, const void* qkv,
                                const int* seq_lens, void* out, float* lse,
                                int B, int S, int heads, hipStream_t stream);
// delta is workspace; dqkv is written whole, no part of it beforehand
void bagua_attention_bwd_launch(int dtype, const void* dout, const void* qkv,
                                const void* out, const float* lse,
                                const int* seq_lens, float* delta, void* dqkv,
                                int B, int S, int heads, hipStream_t stream);

}  // extern "C"
