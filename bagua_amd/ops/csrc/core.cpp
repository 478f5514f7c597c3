// bagua_amd._C — native core: RCCL communicator over xGMI + CDNA4 kernel
// bindings.
//
// MI355X-native replacement for the reference's Rust core
// (bagua-core-internal/src/communicators/mod.rs:25-1155 — which went
// through Aluminum to NCCL). Here RCCL is called directly: thin typed
// wrappers, grouped p2p, and collectives enqueued on the caller-owned
// high-priority HIP stream. No background thread — enqueue-only calls are
// scheduled from Python on the comm stream (see bagua_amd/backend.py).

#include <torch/extension.h>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPStream.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

// kernels.hip launchers
extern "C" {
void bagua_ew_launch(int op, int dtype, void* x, const void* y, float f,
                     size_t n, hipStream_t stream);
void bagua_async_avg_launch(int dtype, void* x, const void* reduced,
                            const void* x_copy, float nranks, size_t n,
                            hipStream_t stream);
void bagua_reduce_chunk_launch(int dtype, void* x, int num_chunks,
                               int target_chunk, int average, size_t chunk,
                               hipStream_t stream);
void bagua_compress_launch(int dtype, const void* x, uint8_t* out,
                           uint32_t* scratch, uint32_t* partials,
                           size_t chunk, size_t chunk_stride,
                           int num_chunks_total, int chunk_begin,
                           int chunk_count, hipStream_t stream);
void bagua_decompress_launch(int dtype, const uint8_t* in, void* x,
                             size_t chunk, size_t chunk_stride,
                             int chunk_begin, int chunk_count,
                             hipStream_t stream);
void bagua_dequant_reduce_launch(int dtype, const uint8_t* in, void* x,
                                 size_t chunk, size_t chunk_stride,
                                 int num_chunks, int target_chunk,
                                 int average, hipStream_t stream);
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
void bagua_fused_sgd_mixed_launch(void* p, const void* g, float* master,
                                  float* m, float lr, float momentum,
                                  float dampening, float weight_decay,
                                  int nesterov, int momentum_initialized,
                                  size_t n, hipStream_t stream);
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
}

// moe_kernels.hip launchers
extern "C" {
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
}

// epilogue_kernels.hip launchers
extern "C" {
size_t bagua_epi_partial_rows(int dtype, size_t work_rows, int C);
void bagua_epi_bias_relu_launch(int dtype, void* x, const void* bias,
                                size_t rows, int C, hipStream_t stream);
void bagua_epi_bias_relu_pool_launch(int dtype, void* x, const void* bias,
                                     void* p, size_t orows, int Wo, int C,
                                     hipStream_t stream);
void bagua_epi_relu_bwd_launch(int dtype, const void* g, const void* y,
                               void* dx, float* partial, void* db,
                               size_t rows, int C, hipStream_t stream);
void bagua_epi_pool_relu_bwd_launch(int dtype, const void* g, const void* y,
                                    void* dx, float* partial, void* db,
                                    size_t orows, int Wo, int C,
                                    hipStream_t stream);
}

// first_conv_kernels.hip launchers
extern "C" {
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
}

#define HIP_CHECK(cmd)                                                    \
  do {                                                                    \
    hipError_t e = (cmd);                                                 \
    if (e != hipSuccess)                                                  \
      throw std::runtime_error(std::string("HIP error: ") +              \
                               hipGetErrorString(e));                     \
  } while (0)

#define NCCL_CHECK(cmd)                                                   \
  do {                                                                    \
    ncclResult_t r = (cmd);                                               \
    if (r != ncclSuccess)                                                 \
      throw std::runtime_error(std::string("RCCL error: ") +             \
                               ncclGetErrorString(r));                    \
  } while (0)

namespace {

ncclDataType_t nccl_dtype(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return ncclFloat32;
    case at::kHalf: return ncclFloat16;
    case at::kBFloat16: return ncclBfloat16;
    case at::kByte: return ncclUint8;
    case at::kLong: return ncclInt64;
    case at::kInt: return ncclInt32;
    case at::kDouble: return ncclFloat64;
    default:
      throw std::runtime_error("unsupported dtype for RCCL collective");
  }
}

// bagua_amd ReduceOp values (communication.py:ReduceOp)
ncclRedOp_t nccl_op(int op) {
  switch (op) {
    case 0: return ncclSum;
    case 1: return ncclProd;
    case 2: return ncclMin;
    case 3: return ncclMax;
    case 10: return ncclAvg;
    default:
      throw std::runtime_error("ReduceOp not supported by RCCL backend");
  }
}

// kernel dtype code: 0=f32 1=f16 2=bf16
int kernel_dtype(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kHalf: return 1;
    case at::kBFloat16: return 2;
    default:
      throw std::runtime_error("kernel supports f32/f16/bf16 only");
  }
}

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_device_contig(const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), "expected a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), "expected a contiguous tensor");
}

}  // namespace

// ---------------------------------------------------------------------------
// Communicator
// ---------------------------------------------------------------------------

class Communicator {
 public:
  Communicator(int rank, int nranks, int device, uintptr_t stream,
               const std::string& uid_bytes)
      : rank_(rank), nranks_(nranks), device_(device),
        stream_((hipStream_t)stream) {
    TORCH_CHECK(uid_bytes.size() == sizeof(ncclUniqueId),
                "bad nccl unique id size");
    HIP_CHECK(hipSetDevice(device_));
    ncclUniqueId id;
    std::memcpy(&id, uid_bytes.data(), sizeof(id));
    NCCL_CHECK(ncclCommInitRank(&comm_, nranks_, id, rank_));
  }

  ~Communicator() {
    if (comm_) ncclCommDestroy(comm_);
  }

  int rank() const { return rank_; }
  int nranks() const { return nranks_; }

  void abort() {
    if (comm_) {
      ncclCommAbort(comm_);
      comm_ = nullptr;
    }
  }

  // graceful teardown from a known-good thread (deinit_process_group);
  // relying on GC to run ~Communicator from an arbitrary thread leaks
  // RCCL state in long-lived multi-model processes
  void destroy() {
    if (comm_) {
      ncclCommDestroy(comm_);
      comm_ = nullptr;
    }
  }

  ncclComm_t raw() const { return comm_; }

  void group_start() { NCCL_CHECK(ncclGroupStart()); }
  void group_end() { NCCL_CHECK(ncclGroupEnd()); }

  // world-size-1 identity fast paths: a single-rank RCCL reduce still
  // launches real kernels (~150us per 32 MiB bucket measured); these
  // collectives are mathematically identity at nranks==1.
  bool single_() const { return nranks_ == 1; }
  void copy_(at::Tensor& dst, const at::Tensor& src) {
    if (dst.data_ptr() != src.data_ptr())
      HIP_CHECK(hipMemcpyAsync(dst.data_ptr(), src.data_ptr(),
                               src.numel() * src.element_size(),
                               hipMemcpyDeviceToDevice, stream_));
  }

  // -- collectives (all enqueue on stream_, non-blocking host) ----------
  void allreduce_inplace(at::Tensor t, int op) {
    if (single_()) return;
    check_device_contig(t);
    NCCL_CHECK(ncclAllReduce(t.data_ptr(), t.data_ptr(), t.numel(),
                             nccl_dtype(t), nccl_op(op), comm_, stream_));
  }

  void allreduce(at::Tensor send, at::Tensor recv, int op) {
    if (single_()) { copy_(recv, send); return; }
    check_device_contig(send);
    check_device_contig(recv);
    NCCL_CHECK(ncclAllReduce(send.data_ptr(), recv.data_ptr(), send.numel(),
                             nccl_dtype(send), nccl_op(op), comm_, stream_));
  }

  void reduce_inplace(at::Tensor t, int dst, int op) {
    if (single_()) return;
    check_device_contig(t);
    NCCL_CHECK(ncclReduce(t.data_ptr(), t.data_ptr(), t.numel(),
                          nccl_dtype(t), nccl_op(op), dst, comm_, stream_));
  }

  void broadcast(at::Tensor t, int src) {
    if (single_()) return;
    check_device_contig(t);
    NCCL_CHECK(ncclBroadcast(t.data_ptr(), t.data_ptr(), t.numel(),
                             nccl_dtype(t), src, comm_, stream_));
  }

  void allgather(at::Tensor send, at::Tensor recv) {
    if (single_()) { copy_(recv, send); return; }
    check_device_contig(send);
    check_device_contig(recv);
    TORCH_CHECK(recv.numel() == send.numel() * nranks_,
                "allgather size mismatch");
    NCCL_CHECK(ncclAllGather(send.data_ptr(), recv.data_ptr(), send.numel(),
                             nccl_dtype(send), comm_, stream_));
  }

  void allgather_inplace(at::Tensor t) {
    if (single_()) return;
    check_device_contig(t);
    TORCH_CHECK(t.numel() % nranks_ == 0, "allgather_inplace size");
    size_t chunk = t.numel() / nranks_;
    char* base = (char*)t.data_ptr();
    char* own = base + rank_ * chunk * t.element_size();
    NCCL_CHECK(ncclAllGather(own, base, chunk, nccl_dtype(t), comm_,
                             stream_));
  }

  void reduce_scatter(at::Tensor send, at::Tensor recv, int op) {
    if (single_()) { copy_(recv, send); return; }
    check_device_contig(send);
    check_device_contig(recv);
    NCCL_CHECK(ncclReduceScatter(send.data_ptr(), recv.data_ptr(),
                                 recv.numel(), nccl_dtype(send), nccl_op(op),
                                 comm_, stream_));
  }

  void reduce_scatter_inplace(at::Tensor t, int op) {
    if (single_()) return;
    check_device_contig(t);
    TORCH_CHECK(t.numel() % nranks_ == 0, "reduce_scatter_inplace size");
    size_t chunk = t.numel() / nranks_;
    char* base = (char*)t.data_ptr();
    char* own = base + rank_ * chunk * t.element_size();
    NCCL_CHECK(ncclReduceScatter(base, own, chunk, nccl_dtype(t),
                                 nccl_op(op), comm_, stream_));
  }

  void alltoall(at::Tensor send, at::Tensor recv) {
    if (single_()) { copy_(recv, send); return; }
    check_device_contig(send);
    check_device_contig(recv);
    TORCH_CHECK(send.numel() % nranks_ == 0, "alltoall size");
    NCCL_CHECK(ncclAllToAll(send.data_ptr(), recv.data_ptr(),
                            send.numel() / nranks_, nccl_dtype(send), comm_,
                            stream_));
  }

  void alltoall_inplace(at::Tensor t) {
    if (single_()) return;
    // RCCL alltoall is not in-place capable; bounce through a PERSISTENT
    // per-communicator scratch buffer. A transient at::empty_like here
    // would be allocated on the caller's ambient (compute) stream but
    // consumed on the comm stream, and freeing it on return lets the
    // caching allocator recycle the block under the in-flight alltoall.
    // Keeping the scratch alive for the communicator's lifetime removes
    // the hazard (and the per-call allocation).
    check_device_contig(t);
    size_t need = (size_t)t.numel() * t.element_size();
    if (!a2a_scratch_.defined() ||
        (size_t)a2a_scratch_.numel() < need ||
        a2a_scratch_.device() != t.device()) {
      if (a2a_scratch_.defined()) {
        // the old scratch may still be in flight on the comm stream;
        // fence before releasing it back to the allocator (rare path:
        // only when the message size grows).
        HIP_CHECK(hipStreamSynchronize(stream_));
      }
      a2a_scratch_ = at::empty(
          {(int64_t)need}, t.options().dtype(at::kByte));
    }
    at::Tensor tmp = a2a_scratch_.narrow(0, 0, need).view(t.scalar_type());
    alltoall(t, tmp);
    HIP_CHECK(hipMemcpyAsync(t.data_ptr(), tmp.data_ptr(),
                             t.numel() * t.element_size(),
                             hipMemcpyDeviceToDevice, stream_));
  }

  void alltoall_v(at::Tensor send, std::vector<int64_t> send_counts,
                  std::vector<int64_t> send_displs, at::Tensor recv,
                  std::vector<int64_t> recv_counts,
                  std::vector<int64_t> recv_displs) {
    check_device_contig(send);
    check_device_contig(recv);
    std::vector<size_t> sc(send_counts.begin(), send_counts.end());
    std::vector<size_t> sd(send_displs.begin(), send_displs.end());
    std::vector<size_t> rc(recv_counts.begin(), recv_counts.end());
    std::vector<size_t> rd(recv_displs.begin(), recv_displs.end());
    NCCL_CHECK(ncclAllToAllv(send.data_ptr(), sc.data(), sd.data(),
                             recv.data_ptr(), rc.data(), rd.data(),
                             nccl_dtype(send), comm_, stream_));
  }

  void send(at::Tensor t, int dst) {
    check_device_contig(t);
    NCCL_CHECK(ncclSend(t.data_ptr(), t.numel(), nccl_dtype(t), dst, comm_,
                        stream_));
  }

  void recv(at::Tensor t, int src) {
    check_device_contig(t);
    NCCL_CHECK(ncclRecv(t.data_ptr(), t.numel(), nccl_dtype(t), src, comm_,
                        stream_));
  }

  void gather(at::Tensor send, at::Tensor recv, int dst) {
    check_device_contig(send);
    group_start();
    if (rank_ == dst) {
      check_device_contig(recv);
      size_t chunk = recv.numel() / nranks_;
      char* base = (char*)recv.data_ptr();
      for (int r = 0; r < nranks_; ++r) {
        NCCL_CHECK(ncclRecv(base + r * chunk * recv.element_size(), chunk,
                            nccl_dtype(recv), r, comm_, stream_));
      }
    }
    NCCL_CHECK(ncclSend(send.data_ptr(), send.numel(), nccl_dtype(send), dst,
                        comm_, stream_));
    group_end();
  }

  void gather_inplace(at::Tensor t, int64_t count, int dst) {
    check_device_contig(t);
    char* base = (char*)t.data_ptr();
    char* own = base + rank_ * count * t.element_size();
    group_start();
    if (rank_ == dst) {
      for (int r = 0; r < nranks_; ++r) {
        if (r == dst) continue;
        NCCL_CHECK(ncclRecv(base + r * count * t.element_size(), count,
                            nccl_dtype(t), r, comm_, stream_));
      }
    } else {
      NCCL_CHECK(ncclSend(own, count, nccl_dtype(t), dst, comm_, stream_));
    }
    group_end();
  }

  void scatter(at::Tensor send, at::Tensor recv, int src) {
    check_device_contig(recv);
    group_start();
    if (rank_ == src) {
      check_device_contig(send);
      size_t chunk = send.numel() / nranks_;
      char* base = (char*)send.data_ptr();
      for (int r = 0; r < nranks_; ++r) {
        NCCL_CHECK(ncclSend(base + r * chunk * send.element_size(), chunk,
                            nccl_dtype(send), r, comm_, stream_));
      }
    }
    NCCL_CHECK(ncclRecv(recv.data_ptr(), recv.numel(), nccl_dtype(recv), src,
                        comm_, stream_));
    group_end();
  }

  void scatter_inplace(at::Tensor t, int64_t count, int src) {
    check_device_contig(t);
    char* base = (char*)t.data_ptr();
    char* own = base + rank_ * count * t.element_size();
    group_start();
    if (rank_ == src) {
      for (int r = 0; r < nranks_; ++r) {
        if (r == src) continue;
        NCCL_CHECK(ncclSend(base + r * count * t.element_size(), count,
                            nccl_dtype(t), r, comm_, stream_));
      }
    } else {
      NCCL_CHECK(ncclRecv(own, count, nccl_dtype(t), src, comm_, stream_));
    }
    group_end();
  }

 private:
  int rank_, nranks_, device_;
  hipStream_t stream_;
  ncclComm_t comm_ = nullptr;
  at::Tensor a2a_scratch_;  // persistent alltoall_inplace bounce buffer
};

static int64_t compressed_chunk_stride(int64_t chunk);

// ---------------------------------------------------------------------------
// BucketExecutor — native centralized-op executor + watchdog.
//
// MI355X re-design of the reference's background scheduler
// (bagua-core-internal/src/lib.rs:209-338): instead of a comm worker
// thread draining a channel, the autograd hook thread calls execute()
// directly — RCCL calls are enqueue-only, so a thread handoff would only
// add latency. The GIL is released for the whole bucket execution, all
// work lands on the dedicated comm stream, and completion is tracked by
// events the compute stream waits on (no host syncs in the hot path).
// The watchdog thread reproduces comm_monitor (lib.rs:255-265): if a
// scheduled bucket has not completed within 300 s it aborts the
// communicator and screams, so a wedged collective cannot hang training
// silently.
// ---------------------------------------------------------------------------

class BucketExecutor {
 public:
  struct Bucket {
    at::Tensor flat;
    bool compressed = false;
    bool scattergather = false;
    bool average = true;
    bool hierarchical = false;
    at::Tensor wire;       // compressed wire buffer
    at::Tensor wire_tmp;   // alltoall bounce
    at::Tensor scratch;    // minmax result (uint32 x 2*chunks)
    at::Tensor partials;   // per-block minmax partials
  };

  BucketExecutor(std::shared_ptr<Communicator> global,
                 std::shared_ptr<Communicator> intra,
                 std::shared_ptr<Communicator> inter, uintptr_t stream)
      : global_(std::move(global)), intra_(std::move(intra)),
        inter_(std::move(inter)), stream_((hipStream_t)stream),
        stop_(false) {
    watchdog_ = std::thread([this] { this->watch(); });
  }

  ~BucketExecutor() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    if (watchdog_.joinable()) watchdog_.join();
    for (auto ev : event_pool_) hipEventDestroy(ev);
    for (auto& p : inflight_) hipEventDestroy(p.first);
  }

  int register_bucket(at::Tensor flat, bool compressed, bool scattergather,
                      bool average, bool hierarchical) {
    check_device_contig(flat);
    Bucket b;
    b.flat = flat;
    b.compressed = compressed;
    b.scattergather = scattergather;
    b.average = average;
    b.hierarchical = hierarchical;
    if (compressed) {
      Communicator* c = inner_comm(hierarchical);
      if (c != nullptr) {  // null on hierarchical non-leader ranks
        int n = c->nranks();
        TORCH_CHECK(flat.numel() % n == 0, "bucket not padded to nranks");
        int64_t chunk = flat.numel() / n;
        int64_t stride = compressed_chunk_stride(chunk);
        b.wire = at::empty({stride * n}, flat.options().dtype(at::kByte));
        b.wire_tmp = at::empty_like(b.wire);
        b.scratch = at::empty({2 * n}, flat.options().dtype(at::kInt));
        b.partials = at::empty({2 * 512 * n},
                               flat.options().dtype(at::kInt));
      }
    }
    buckets_.push_back(std::move(b));
    return (int)buckets_.size() - 1;
  }

  void execute(int idx, const std::vector<uintptr_t>& ready_events) {
    py::gil_scoped_release nogil;
    Bucket& b = buckets_.at(idx);
    for (uintptr_t ev : ready_events)
      HIP_CHECK(hipStreamWaitEvent(stream_, (hipEvent_t)ev, 0));

    bool multi_node = b.hierarchical && intra_ &&
                      intra_->nranks() < global_->nranks();
    Communicator* comm = multi_node ? inter_.get() : global_.get();

    if (multi_node)
      intra_->reduce_inplace(b.flat, 0, b.average ? 10 : 0);
    if (!multi_node || intra_->rank() == 0) {
      TORCH_CHECK(comm != nullptr, "leader rank missing inter communicator");
      if (b.compressed)
        run_compressed(b, comm);
      else if (b.scattergather)
        run_scattergather(b, comm);
      else
        comm->allreduce_inplace(b.flat, b.average ? 10 : 0);
    }
    if (multi_node) intra_->broadcast(b.flat, 0);

    hipEvent_t done = get_event();
    HIP_CHECK(hipEventRecord(done, stream_));
    {
      std::lock_guard<std::mutex> g(mu_);
      inflight_.emplace_back(done, std::chrono::steady_clock::now());
    }
  }

  // make the given (compute) stream wait on all scheduled comm; recycles
  // completed events. GPU-side only — never blocks the host.
  void wait_pending(uintptr_t compute_stream) {
    py::gil_scoped_release nogil;
    std::lock_guard<std::mutex> g(mu_);
    for (auto& p : inflight_) {
      HIP_CHECK(hipStreamWaitEvent((hipStream_t)compute_stream, p.first,
                                   0));
      event_pool_.push_back(p.first);
    }
    inflight_.clear();
  }

  void synchronize() {
    py::gil_scoped_release nogil;
    HIP_CHECK(hipStreamSynchronize(stream_));
    std::lock_guard<std::mutex> g(mu_);
    for (auto& p : inflight_) event_pool_.push_back(p.first);
    inflight_.clear();
  }

  void clear_buckets() { buckets_.clear(); }

 private:
  Communicator* inner_comm(bool hierarchical) {
    bool multi_node = hierarchical && intra_ &&
                      intra_->nranks() < global_->nranks();
    if (!multi_node) return global_.get();
    return inter_ ? inter_.get() : nullptr;
  }

  void run_scattergather(Bucket& b, Communicator* comm) {
    int n = comm->nranks();
    comm->alltoall_inplace(b.flat);
    bagua_reduce_chunk_launch(kernel_dtype(b.flat), b.flat.data_ptr(), n,
                              comm->rank(), b.average ? 1 : 0,
                              b.flat.numel() / n, stream_);
    comm->allgather_inplace(b.flat);
  }

  void run_compressed(Bucket& b, Communicator* comm) {
    // ByteGrad wire protocol (reference:
    // comm_ops/centralized_low_precision_synchronous.rs:16-74)
    int n = comm->nranks();
    int rank = comm->rank();
    int64_t chunk = b.flat.numel() / n;
    int64_t stride = compressed_chunk_stride(chunk);
    int dt = kernel_dtype(b.flat);
    auto* wire = (uint8_t*)b.wire.data_ptr();
    auto* scratch = (uint32_t*)b.scratch.data_ptr();
    auto* partials = (uint32_t*)b.partials.data_ptr();

    bagua_compress_launch(dt, b.flat.data_ptr(), wire, scratch, partials,
                          chunk, stride, n, 0, n, stream_);
    comm->alltoall(b.wire, b.wire_tmp);
    std::swap(b.wire, b.wire_tmp);
    wire = (uint8_t*)b.wire.data_ptr();
    // fused dequantize+reduce straight from the wire into the target
    // chunk: the non-target chunks were only reduction inputs, so the
    // old decompress-then-reduce pair paid ~2 extra bucket passes of
    // HBM traffic for nothing (bitwise-identical result — the kernel
    // rounds through T between dequantize and accumulate)
    if (n <= 64) {
      bagua_dequant_reduce_launch(dt, wire, b.flat.data_ptr(), chunk,
                                  stride, n, rank, b.average ? 1 : 0,
                                  stream_);
    } else {  // beyond the kernel's LDS param table: unfused fallback
      bagua_decompress_launch(dt, wire, b.flat.data_ptr(), chunk, stride,
                              0, n, stream_);
      bagua_reduce_chunk_launch(dt, b.flat.data_ptr(), n, rank,
                                b.average ? 1 : 0, chunk, stream_);
    }
    bagua_compress_launch(dt, b.flat.data_ptr(), wire, scratch, partials,
                          chunk, stride, n, rank, 1, stream_);
    // in-place allgather of the rank's wire chunk (identity at n==1)
    if (n > 1) {
      char* base = (char*)wire;
      char* own = base + (int64_t)rank * stride;
      NCCL_CHECK(ncclAllGather(own, base, stride, ncclUint8,
                               comm->raw(), stream_));
    }
    bagua_decompress_launch(dt, wire, b.flat.data_ptr(), chunk, stride, 0,
                            n, stream_);
  }

  hipEvent_t get_event() {
    std::lock_guard<std::mutex> g(mu_);
    if (!event_pool_.empty()) {
      hipEvent_t ev = event_pool_.back();
      event_pool_.pop_back();
      return ev;
    }
    hipEvent_t ev;
    HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return ev;
  }

  void watch() {
    using namespace std::chrono;
    std::unique_lock<std::mutex> lk(mu_);
    while (!stop_) {
      cv_.wait_for(lk, seconds(10));
      if (stop_) break;
      auto now = steady_clock::now();
      for (auto& p : inflight_) {
        if (hipEventQuery(p.first) == hipSuccess) continue;
        if (duration_cast<seconds>(now - p.second).count() > 300) {
          fprintf(stderr,
                  "[bagua_amd] FATAL: a scheduled communication has been "
                  "running for >300s; aborting ALL communicators\n");
          fflush(stderr);
          lk.unlock();
          // in hierarchical mode the wedged collective can live on ANY of
          // the three communicators — abort them all so no intra/inter
          // collective keeps the ranks pinned
          global_->abort();
          if (intra_) intra_->abort();
          if (inter_) inter_->abort();
          lk.lock();
          break;
        }
      }
    }
  }

  std::shared_ptr<Communicator> global_, intra_, inter_;
  hipStream_t stream_;
  std::vector<Bucket> buckets_;
  std::vector<hipEvent_t> event_pool_;
  std::vector<std::pair<hipEvent_t,
                        std::chrono::steady_clock::time_point>> inflight_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::thread watchdog_;
  bool stop_;
};

// ---------------------------------------------------------------------------
// Direct one-hop p2p alltoall over xGMI (SURVEY hard part #4 prototype).
//
// The 8-GPU MI355X node is fully connected (7 xGMI links per GPU), so
// the natural alltoall is each rank PULLING its chunk from every peer's
// exported buffer in one hop — no ring, no proxy. Buffers and a
// fine-grained flag array are exported with hipIpcGetMemHandle and
// opened by peers; rounds are ordered by a device-side sequence-number
// barrier (kernels.hip p2p_barrier_kernel) because re-recorded IPC
// events race across processes. The pulls are plain stream-ordered D2D
// copies (SDMA engines move them over the direct link).
//
// Opt-in (BAGUA_P2P_ALLTOALL=1 wires it into the scattergather/ByteGrad
// chunk exchange); default stays on ncclAllToAll.
// ---------------------------------------------------------------------------

extern "C" void bagua_p2p_barrier_launch(void* peer_flags_dev_array,
                                         void* my_flags, int rank,
                                         int nranks,
                                         unsigned long long seq,
                                         hipStream_t stream);

class P2PAlltoAll {
 public:
  P2PAlltoAll(int rank, int nranks, uintptr_t stream, int64_t capacity)
      : rank_(rank), nranks_(nranks), stream_((hipStream_t)stream),
        capacity_(capacity) {
    TORCH_CHECK(nranks_ >= 1 && nranks_ <= 64, "p2p alltoall: 1..64 ranks");
    HIP_CHECK(hipMalloc(&send_, capacity_));
    HIP_CHECK(hipMalloc(&recv_, capacity_));
    // flags must be FINE-GRAINED for cross-device visibility of the
    // barrier stores over xGMI
    HIP_CHECK(hipExtMallocWithFlags(
        (void**)&flags_, nranks_ * sizeof(unsigned long long),
        hipDeviceMallocFinegrained));
    HIP_CHECK(hipMemset((void*)flags_, 0,
                        nranks_ * sizeof(unsigned long long)));
    HIP_CHECK(hipMalloc(&d_peer_flags_, nranks_ * sizeof(void*)));
    peer_send_.assign(nranks_, nullptr);
    peer_flags_.assign(nranks_, nullptr);
  }

  ~P2PAlltoAll() {
    for (int p = 0; p < nranks_; ++p) {
      if (p != rank_ && peer_send_[p]) hipIpcCloseMemHandle(peer_send_[p]);
      if (p != rank_ && peer_flags_[p])
        hipIpcCloseMemHandle((void*)peer_flags_[p]);
    }
    hipFree(send_);
    hipFree(recv_);
    hipFree((void*)flags_);
    hipFree(d_peer_flags_);
  }

  // serialized (send handle || flags handle) for the store exchange
  py::bytes handles() {
    hipIpcMemHandle_t h[2];
    HIP_CHECK(hipIpcGetMemHandle(&h[0], send_));
    HIP_CHECK(hipIpcGetMemHandle(&h[1], (void*)flags_));
    return py::bytes((const char*)h, sizeof(h));
  }

  void connect(const std::vector<std::string>& peer_handles) {
    TORCH_CHECK((int)peer_handles.size() == nranks_,
                "need one handle blob per rank");
    for (int p = 0; p < nranks_; ++p) {
      if (p == rank_) {
        peer_send_[p] = send_;
        peer_flags_[p] = flags_;
        continue;
      }
      TORCH_CHECK(peer_handles[p].size() == 2 * sizeof(hipIpcMemHandle_t),
                  "bad handle blob size");
      hipIpcMemHandle_t h[2];
      std::memcpy(h, peer_handles[p].data(), sizeof(h));
      void* ps = nullptr;
      void* pf = nullptr;
      HIP_CHECK(hipIpcOpenMemHandle(&ps, h[0],
                                    hipIpcMemLazyEnablePeerAccess));
      HIP_CHECK(hipIpcOpenMemHandle(&pf, h[1],
                                    hipIpcMemLazyEnablePeerAccess));
      peer_send_[p] = ps;
      peer_flags_[p] = (unsigned long long*)pf;
    }
    HIP_CHECK(hipMemcpy(d_peer_flags_, peer_flags_.data(),
                        nranks_ * sizeof(void*), hipMemcpyHostToDevice));
    connected_ = true;
  }

  int64_t capacity() const { return capacity_; }

  void alltoall(at::Tensor input, at::Tensor output) {
    py::gil_scoped_release nogil;
    exchange_(input, output, /*allgather=*/false);
  }

  // one-hop allgather: every rank publishes ONLY its own chunk (at its
  // rank offset in the exported buffer) and pulls chunk p from peer p's
  // own-chunk slot. input/output are the FULL buffer; input's rank-chunk
  // is the contribution (ncclAllGather-inplace shape).
  void allgather_inplace(at::Tensor t) {
    py::gil_scoped_release nogil;
    exchange_(t, t, /*allgather=*/true);
  }

 private:
  void exchange_(at::Tensor input, at::Tensor output, bool allgather) {
    TORCH_CHECK(connected_, "p2p exchange used before connect()");
    check_device_contig(input);
    check_device_contig(output);
    int64_t bytes = input.numel() * input.element_size();
    TORCH_CHECK(output.numel() * output.element_size() == bytes,
                "p2p exchange size mismatch");
    TORCH_CHECK(bytes % nranks_ == 0, "p2p exchange: not divisible");
    TORCH_CHECK(bytes <= capacity_, "p2p exchange: exceeds capacity");
    int64_t chunk = bytes / nranks_;

    if (allgather) {
      // publish my own chunk only
      HIP_CHECK(hipMemcpyAsync(
          (char*)send_ + (int64_t)rank_ * chunk,
          (char*)input.data_ptr() + (int64_t)rank_ * chunk, chunk,
          hipMemcpyDeviceToDevice, stream_));
    } else {
      HIP_CHECK(hipMemcpyAsync(send_, input.data_ptr(), bytes,
                               hipMemcpyDeviceToDevice, stream_));
    }
    // round barrier: all ranks' send buffers are published
    ++seq_;
    bagua_p2p_barrier_launch(d_peer_flags_, (void*)flags_, rank_, nranks_,
                             seq_, stream_);
    for (int p = 0; p < nranks_; ++p) {
      // alltoall pulls MY slice of peer p; allgather pulls peer p's OWN
      // chunk
      int64_t src_off = (allgather ? (int64_t)p : (int64_t)rank_) * chunk;
      HIP_CHECK(hipMemcpyAsync(
          (char*)recv_ + p * chunk, (char*)peer_send_[p] + src_off, chunk,
          hipMemcpyDeviceToDevice, stream_));
    }
    // completion barrier: nobody may overwrite their send buffer until
    // every peer finished pulling this round
    ++seq_;
    bagua_p2p_barrier_launch(d_peer_flags_, (void*)flags_, rank_, nranks_,
                             seq_, stream_);
    HIP_CHECK(hipMemcpyAsync(output.data_ptr(), recv_, bytes,
                             hipMemcpyDeviceToDevice, stream_));
  }

 public:

 private:
  int rank_, nranks_;
  hipStream_t stream_;
  int64_t capacity_;
  void* send_ = nullptr;
  void* recv_ = nullptr;
  unsigned long long* flags_ = nullptr;
  void* d_peer_flags_ = nullptr;
  std::vector<void*> peer_send_;
  std::vector<unsigned long long*> peer_flags_;
  unsigned long long seq_ = 0;
  bool connected_ = false;
};

// ---------------------------------------------------------------------------
// kernel wrappers (run on the CALLER's current torch stream so they are
// ordered with collectives when invoked under torch.cuda.stream(comm))
// ---------------------------------------------------------------------------

static void average_inplace(at::Tensor x, at::Tensor y) {
  check_device_contig(x);
  bagua_ew_launch(0, kernel_dtype(x), x.data_ptr(), y.data_ptr(), 0.f,
                  x.numel(), current_stream());
}
static void add_inplace(at::Tensor x, at::Tensor y) {
  check_device_contig(x);
  bagua_ew_launch(1, kernel_dtype(x), x.data_ptr(), y.data_ptr(), 0.f,
                  x.numel(), current_stream());
}
static void substract_inplace(at::Tensor x, at::Tensor y) {
  check_device_contig(x);
  bagua_ew_launch(2, kernel_dtype(x), x.data_ptr(), y.data_ptr(), 0.f,
                  x.numel(), current_stream());
}
static void addmul_inplace(at::Tensor x, at::Tensor y, double factor) {
  check_device_contig(x);
  bagua_ew_launch(3, kernel_dtype(x), x.data_ptr(), y.data_ptr(),
                  (float)factor, x.numel(), current_stream());
}
static void divide_inplace(at::Tensor x, double divisor) {
  check_device_contig(x);
  bagua_ew_launch(4, kernel_dtype(x), x.data_ptr(), nullptr,
                  1.0f / (float)divisor, x.numel(), current_stream());
}
static void async_model_average(at::Tensor x, at::Tensor reduced,
                                at::Tensor x_copy, double nranks) {
  check_device_contig(x);
  bagua_async_avg_launch(kernel_dtype(x), x.data_ptr(), reduced.data_ptr(),
                         x_copy.data_ptr(), (float)nranks, x.numel(),
                         current_stream());
}
static void reduce_chunk_inplace(at::Tensor x, int64_t num_chunks,
                                 int64_t target_chunk, bool average) {
  check_device_contig(x);
  TORCH_CHECK(x.numel() % num_chunks == 0, "numel must divide num_chunks");
  bagua_reduce_chunk_launch(kernel_dtype(x), x.data_ptr(), (int)num_chunks,
                            (int)target_chunk, average ? 1 : 0,
                            x.numel() / num_chunks, current_stream());
}

static int64_t compressed_chunk_stride(int64_t chunk) {
  int64_t payload = (chunk + 31) / 32 * 32;
  return 32 + payload;
}

static void compress_chunked(at::Tensor flat, at::Tensor out,
                             int64_t num_chunks, int64_t target_chunk) {
  check_device_contig(flat);
  check_device_contig(out);
  TORCH_CHECK(flat.numel() % num_chunks == 0, "chunked size mismatch");
  int64_t chunk = flat.numel() / num_chunks;
  int64_t stride = compressed_chunk_stride(chunk);
  TORCH_CHECK(out.numel() >= stride * num_chunks, "wire buffer too small");
  auto scratch = at::empty({2 * num_chunks},
                           flat.options().dtype(at::kInt));
  int begin = target_chunk >= 0 ? (int)target_chunk : 0;
  int count = target_chunk >= 0 ? 1 : (int)num_chunks;
  auto partials = at::empty({2 * 512 * count},
                            flat.options().dtype(at::kInt));
  bagua_compress_launch(kernel_dtype(flat), flat.data_ptr(),
                        (uint8_t*)out.data_ptr(),
                        (uint32_t*)scratch.data_ptr(),
                        (uint32_t*)partials.data_ptr(), chunk, stride,
                        (int)num_chunks, begin, count, current_stream());
}

static void decompress_chunked(at::Tensor buf, at::Tensor flat,
                               int64_t num_chunks, int64_t target_chunk) {
  check_device_contig(flat);
  check_device_contig(buf);
  TORCH_CHECK(flat.numel() % num_chunks == 0, "chunked size mismatch");
  int64_t chunk = flat.numel() / num_chunks;
  int64_t stride = compressed_chunk_stride(chunk);
  int begin = target_chunk >= 0 ? (int)target_chunk : 0;
  int count = target_chunk >= 0 ? 1 : (int)num_chunks;
  bagua_decompress_launch(kernel_dtype(flat), (uint8_t*)buf.data_ptr(),
                          flat.data_ptr(), chunk, stride, begin, count,
                          current_stream());
}

// fused: flat[target_chunk] = reduce over dequantized wire chunks
static void dequant_reduce(at::Tensor buf, at::Tensor flat,
                           int64_t num_chunks, int64_t target_chunk,
                           bool average) {
  check_device_contig(flat);
  check_device_contig(buf);
  TORCH_CHECK(flat.numel() % num_chunks == 0, "chunked size mismatch");
  TORCH_CHECK(num_chunks <= 64, "dequant_reduce supports <= 64 chunks");
  int64_t chunk = flat.numel() / num_chunks;
  int64_t stride = compressed_chunk_stride(chunk);
  bagua_dequant_reduce_launch(kernel_dtype(flat),
                              (uint8_t*)buf.data_ptr(), flat.data_ptr(),
                              chunk, stride, (int)num_chunks,
                              (int)target_chunk, average ? 1 : 0,
                              current_stream());
}

static void fused_sgd_step(at::Tensor p, at::Tensor g, at::Tensor m,
                           double lr, double momentum, double dampening,
                           double weight_decay, bool nesterov,
                           bool momentum_initialized) {
  check_device_contig(p);
  TORCH_CHECK(p.scalar_type() == at::kFloat, "fused SGD needs f32 master");
  bagua_fused_sgd_launch(
      (float*)p.data_ptr(), (const float*)g.data_ptr(),
      momentum != 0.0 ? (float*)m.data_ptr() : nullptr, (float)lr,
      (float)momentum, (float)dampening, (float)weight_decay,
      nesterov ? 1 : 0, momentum_initialized ? 1 : 0, p.numel(),
      current_stream());
}

static void fused_sgd_mixed_step(at::Tensor p, at::Tensor g,
                                 at::Tensor master, at::Tensor m,
                                 double lr, double momentum,
                                 double dampening, double weight_decay,
                                 bool nesterov, bool momentum_initialized) {
  check_device_contig(p);
  TORCH_CHECK(p.scalar_type() == at::kBFloat16, "params must be bf16");
  TORCH_CHECK(master.scalar_type() == at::kFloat, "master must be f32");
  bagua_fused_sgd_mixed_launch(
      p.data_ptr(), g.data_ptr(), (float*)master.data_ptr(),
      momentum != 0.0 ? (float*)m.data_ptr() : nullptr, (float)lr,
      (float)momentum, (float)dampening, (float)weight_decay,
      nesterov ? 1 : 0, momentum_initialized ? 1 : 0, p.numel(),
      current_stream());
}

static void fused_adam_step(at::Tensor p, at::Tensor g, at::Tensor m,
                            at::Tensor v, int64_t step, double lr,
                            double beta1, double beta2, double eps,
                            double weight_decay, bool adamw) {
  check_device_contig(p);
  TORCH_CHECK(p.scalar_type() == at::kFloat, "fused Adam needs f32 master");
  // in double, cast once: 1.f - (float)pow(beta2, step) and the kernel's
  // former 1.f - beta2 each lose 1.3e-5 relative at beta2 = 0.999 (the
  // subtraction cancels). At step 1 the two errors cancelled each other
  // in v/bc2, later they did not; both are formed here now.
  float bc1 = (float)(1.0 - std::pow(beta1, (double)step));
  float bc2 = (float)(1.0 - std::pow(beta2, (double)step));
  bagua_fused_adam_launch(
      (float*)p.data_ptr(), (const float*)g.data_ptr(),
      (float*)m.data_ptr(), (float*)v.data_ptr(), (float)lr, (float)beta1,
      (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
      (float)weight_decay, adamw ? 1 : 0, bc1, bc2, p.numel(),
      current_stream());
}

// Segmented steps: the flat tensors as above, but the gradient is read
// where it lives. grads[k] covers flat elements [offsets[k], offsets[k+1]);
// None there is a zero gradient.
struct GradSegments {
  std::vector<const void*> grads;
  std::vector<size_t> begins, numels;
};

static GradSegments check_segments(
    const at::Tensor& p, const std::vector<std::optional<at::Tensor>>& grads,
    const std::vector<int64_t>& offsets) {
  check_device_contig(p);
  TORCH_CHECK(offsets.size() == grads.size() + 1,
              "need len(grads) + 1 offsets");
  TORCH_CHECK(offsets.front() == 0 && offsets.back() == p.numel(),
              "segments must tile [0, numel)");
  GradSegments s;
  for (size_t k = 0; k < grads.size(); ++k) {
    const int64_t n = offsets[k + 1] - offsets[k];
    TORCH_CHECK(n >= 0, "segment offsets must ascend");
    const void* ptr = nullptr;
    if (grads[k].has_value()) {
      const at::Tensor& g = *grads[k];
      check_device_contig(g);
      TORCH_CHECK(g.device() == p.device(), "grad ", k, " on another device");
      TORCH_CHECK(g.scalar_type() == p.scalar_type(), "grad ", k,
                  " dtype differs from the parameters'");
      TORCH_CHECK(g.numel() == n, "grad ", k, " has ", g.numel(),
                  " elements, its segment ", n);
      ptr = g.data_ptr();
    }
    if (n == 0) continue;
    s.grads.push_back(ptr);
    s.begins.push_back((size_t)offsets[k]);
    s.numels.push_back((size_t)n);
  }
  return s;
}

static float* check_flat_state(const std::optional<at::Tensor>& t,
                               const at::Tensor& p, bool needed,
                               const char* what) {
  if (!needed) return nullptr;
  TORCH_CHECK(t.has_value(), what, " is missing");
  check_device_contig(*t);
  TORCH_CHECK(t->device() == p.device() && t->scalar_type() == at::kFloat &&
                  t->numel() == p.numel(),
              what, " must be f32, on the parameters' device and of their "
              "size");
  return (float*)t->data_ptr();
}

static void fused_sgd_step_segments(
    at::Tensor p, std::vector<std::optional<at::Tensor>> grads,
    std::vector<int64_t> offsets, std::optional<at::Tensor> m, double lr,
    double momentum, double dampening, double weight_decay, bool nesterov,
    bool momentum_initialized) {
  TORCH_CHECK(p.scalar_type() == at::kFloat, "fused SGD needs f32 master");
  const GradSegments s = check_segments(p, grads, offsets);
  float* mp = check_flat_state(m, p, momentum != 0.0, "momentum buffer");
  bagua_fused_sgd_segments_launch(
      (float*)p.data_ptr(), mp, (float)lr, (float)momentum, (float)dampening,
      (float)weight_decay, nesterov ? 1 : 0, momentum_initialized ? 1 : 0,
      s.grads.data(), s.begins.data(), s.numels.data(), s.grads.size(),
      current_stream());
}

static void fused_sgd_mixed_step_segments(
    at::Tensor p, std::vector<std::optional<at::Tensor>> grads,
    std::vector<int64_t> offsets, at::Tensor master,
    std::optional<at::Tensor> m, double lr, double momentum,
    double dampening, double weight_decay, bool nesterov,
    bool momentum_initialized) {
  TORCH_CHECK(p.scalar_type() == at::kBFloat16, "params must be bf16");
  const GradSegments s = check_segments(p, grads, offsets);
  float* master_p = check_flat_state(master, p, true, "master");
  float* mp = check_flat_state(m, p, momentum != 0.0, "momentum buffer");
  bagua_fused_sgd_mixed_segments_launch(
      p.data_ptr(), master_p, mp, (float)lr, (float)momentum,
      (float)dampening, (float)weight_decay, nesterov ? 1 : 0,
      momentum_initialized ? 1 : 0, s.grads.data(), s.begins.data(),
      s.numels.data(), s.grads.size(), current_stream());
}

static void fused_adam_step_segments(
    at::Tensor p, std::vector<std::optional<at::Tensor>> grads,
    std::vector<int64_t> offsets, at::Tensor m, at::Tensor v, int64_t step,
    double lr, double beta1, double beta2, double eps, double weight_decay,
    bool adamw) {
  TORCH_CHECK(p.scalar_type() == at::kFloat, "fused Adam needs f32 master");
  const GradSegments s = check_segments(p, grads, offsets);
  float* mp = check_flat_state(m, p, true, "exp_avg");
  float* vp = check_flat_state(v, p, true, "exp_avg_sq");
  // bias corrections and 1 - beta as in fused_adam_step
  float bc1 = (float)(1.0 - std::pow(beta1, (double)step));
  float bc2 = (float)(1.0 - std::pow(beta2, (double)step));
  bagua_fused_adam_segments_launch(
      (float*)p.data_ptr(), mp, vp, (float)lr, (float)beta1, (float)beta2,
      (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
      (float)weight_decay, adamw ? 1 : 0, bc1, bc2, s.grads.data(),
      s.begins.data(), s.numels.data(), s.grads.size(), current_stream());
}

// ---------------------------------------------------------------------------
// index-based MoE routing (moe_kernels.hip)
// ---------------------------------------------------------------------------

static constexpr int64_t kInt31 = (int64_t)1 << 31;

static void check_moe_index(const at::Tensor& t, const char* what) {
  check_device_contig(t);
  TORCH_CHECK(t.scalar_type() == at::kInt, what, " must be int32");
}

static void check_moe_weights(const at::Tensor& t, int64_t k, int64_t S) {
  check_device_contig(t);
  TORCH_CHECK(t.scalar_type() == at::kFloat, "weights must be float32");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == k && t.size(1) == S,
              "weights must have shape (k, S)");
}

// dest (k, S) with k in {1, 2}; returns k
static int64_t check_moe_dest(const at::Tensor& dest) {
  check_moe_index(dest, "dest");
  TORCH_CHECK(dest.dim() == 2 && (dest.size(0) == 1 || dest.size(0) == 2),
              "dest must have shape (k, S) with k in {1, 2}");
  TORCH_CHECK(dest.numel() < kInt31, "S * k must be below 2^31");
  return dest.size(0);
}

static void check_moe_rows(const at::Tensor& t, const char* what) {
  check_device_contig(t);
  TORCH_CHECK(t.dim() == 2, what, " must be 2-d (rows, M)");
  TORCH_CHECK(t.size(0) < kInt31 && t.size(1) < kInt31, what,
              ": rows and M must be below 2^31");
}

static void moe_assign_slots(at::Tensor expert, int64_t num_experts,
                             int64_t capacity,
                             std::optional<at::Tensor> base, at::Tensor slot,
                             at::Tensor counts, at::Tensor src) {
  check_moe_index(expert, "expert");
  check_moe_index(slot, "slot");
  check_moe_index(counts, "counts");
  check_moe_index(src, "src");
  TORCH_CHECK(expert.dim() == 1, "expert must be 1-d");
  // the per-expert counters of a block live in LDS
  TORCH_CHECK(num_experts >= 1 && num_experts <= 8192,
              "moe_assign_slots supports 1..8192 experts");
  TORCH_CHECK(capacity >= 1, "capacity must be positive");
  TORCH_CHECK(expert.numel() < kInt31 / 2, "S * k must be below 2^31");
  TORCH_CHECK(num_experts * capacity < kInt31,
              "num_experts * capacity must be below 2^31");
  TORCH_CHECK(slot.numel() == expert.numel(), "slot size mismatch");
  TORCH_CHECK(counts.numel() == num_experts, "counts size mismatch");
  TORCH_CHECK(src.numel() == num_experts * capacity, "src size mismatch");
  const int* base_ptr = nullptr;
  if (base.has_value()) {
    check_moe_index(*base, "base");
    TORCH_CHECK(base->numel() == num_experts, "base size mismatch");
    base_ptr = (const int*)base->data_ptr();
  }
  const int S = (int)expert.numel(), E = (int)num_experts;
  auto hist = at::empty({(int64_t)bagua_moe_assign_workspace(S, E)},
                        expert.options());
  bagua_moe_assign_slots_launch(
      (const int*)expert.data_ptr(), S, E, (int)capacity, base_ptr,
      (int*)hist.data_ptr(), (int*)slot.data_ptr(), (int*)counts.data_ptr(),
      (int*)src.data_ptr(), current_stream());
}

static void moe_gather_rows(at::Tensor x, at::Tensor src, at::Tensor out,
                            std::optional<at::Tensor> w,
                            std::optional<at::Tensor> dest) {
  check_moe_rows(x, "x");
  check_moe_rows(out, "out");
  check_moe_index(src, "src");
  TORCH_CHECK(out.scalar_type() == x.scalar_type(), "out dtype mismatch");
  TORCH_CHECK(src.dim() == 1 && out.size(0) == src.numel() &&
                  out.size(1) == x.size(1), "out must be (len(src), M)");
  const int64_t S = x.size(0);
  const float* w_ptr = nullptr;
  const int* dest_ptr = nullptr;
  int64_t k = 1;
  if (w.has_value()) {
    TORCH_CHECK(dest.has_value(), "scaled gather needs dest");
    k = check_moe_dest(*dest);
    TORCH_CHECK(dest->size(1) == S, "dest must have shape (k, S)");
    check_moe_weights(*w, k, S);
    w_ptr = (const float*)w->data_ptr();
    dest_ptr = (const int*)dest->data_ptr();
  }
  bagua_moe_gather_rows_launch(kernel_dtype(x), x.data_ptr(),
                               (const int*)src.data_ptr(), out.data_ptr(),
                               w_ptr, dest_ptr, (int)k, (int)S,
                               (size_t)src.numel(), (int)x.size(1),
                               current_stream());
}

static void moe_combine_rows(at::Tensor eo, at::Tensor dest, at::Tensor out,
                             std::optional<at::Tensor> w) {
  check_moe_rows(eo, "eo");
  check_moe_rows(out, "out");
  const int64_t k = check_moe_dest(dest);
  const int64_t S = dest.size(1);
  TORCH_CHECK(out.scalar_type() == eo.scalar_type(), "out dtype mismatch");
  TORCH_CHECK(out.size(0) == S && out.size(1) == eo.size(1),
              "out must be (S, M)");
  const float* w_ptr = nullptr;
  if (w.has_value()) {
    check_moe_weights(*w, k, S);
    w_ptr = (const float*)w->data_ptr();
  }
  bagua_moe_combine_rows_launch(kernel_dtype(eo), eo.data_ptr(),
                                (const int*)dest.data_ptr(), out.data_ptr(),
                                w_ptr, (int)k, (int)S, (size_t)eo.size(0),
                                (int)eo.size(1), current_stream());
}

static void moe_row_dot(at::Tensor g, at::Tensor eo, at::Tensor dest,
                        at::Tensor gw) {
  check_moe_rows(g, "g");
  check_moe_rows(eo, "eo");
  const int64_t k = check_moe_dest(dest);
  const int64_t S = dest.size(1);
  TORCH_CHECK(g.scalar_type() == eo.scalar_type(), "g/eo dtype mismatch");
  TORCH_CHECK(g.size(0) == S && g.size(1) == eo.size(1),
              "g must be (S, M)");
  check_moe_weights(gw, k, S);
  bagua_moe_row_dot_launch(kernel_dtype(g), g.data_ptr(), eo.data_ptr(),
                           (const int*)dest.data_ptr(),
                           (float*)gw.data_ptr(), (int)k, (int)S,
                           (size_t)eo.size(0), (int)g.size(1),
                           current_stream());
}

// ---------------------------------------------------------------------------
// convolution epilogue (epilogue_kernels.hip): channels-last (N, C, H, W)
// tensors, seen by the kernels as [N*H*W, C]
// ---------------------------------------------------------------------------

// full-size activation of the stage; returns its row count N*H*W
static int64_t check_epi_act(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda(), what, " must be a GPU tensor");
  TORCH_CHECK(t.dim() == 4 &&
                  t.is_contiguous(at::MemoryFormat::ChannelsLast),
              what, " must be 4-d and channels-last contiguous");
  const int64_t vec = 16 / (int64_t)t.element_size();
  const int64_t C = t.size(1);
  TORCH_CHECK(C > 0 && C % vec == 0 && C / vec <= 256, what,
              ": C must be a multiple of ", vec, " and at most ", 256 * vec);
  TORCH_CHECK(((uintptr_t)t.data_ptr() & 15u) == 0, what,
              " must be 16-byte aligned");
  const int64_t rows = t.size(0) * t.size(2) * t.size(3);
  TORCH_CHECK(rows < kInt31, what, ": N*H*W must be below 2^31");
  return rows;
}

static void check_epi_like(const at::Tensor& t, const at::Tensor& ref,
                           const char* what) {
  check_epi_act(t, what);
  TORCH_CHECK(t.sizes() == ref.sizes() &&
                  t.scalar_type() == ref.scalar_type() &&
                  t.device() == ref.device(),
              what, ": shape, dtype or device mismatch");
}

static void check_epi_bias(const at::Tensor& b, const at::Tensor& act,
                           const char* what) {
  check_device_contig(b);
  TORCH_CHECK(b.dim() == 1 && b.size(0) == act.size(1) &&
                  b.scalar_type() == act.scalar_type() &&
                  b.device() == act.device(),
              what, " must be 1-d of C elements, in the activation's dtype "
              "and on its device");
}

// pooled companion of the full-size activation y
static void check_epi_pooled(const at::Tensor& p, const at::Tensor& y,
                             const char* what) {
  TORCH_CHECK(y.size(2) % 2 == 0 && y.size(3) % 2 == 0,
              "pooling needs even H and W");
  check_epi_act(p, what);
  TORCH_CHECK(p.size(0) == y.size(0) && p.size(1) == y.size(1) &&
                  p.size(2) == y.size(2) / 2 && p.size(3) == y.size(3) / 2 &&
                  p.scalar_type() == y.scalar_type() &&
                  p.device() == y.device(),
              what, " must be (N, C, H/2, W/2) in the activation's dtype");
}

// x = relu(x + bias), in place
static void conv_bias_relu_(at::Tensor x, at::Tensor bias) {
  const int64_t rows = check_epi_act(x, "x");
  check_epi_bias(bias, x, "bias");
  bagua_epi_bias_relu_launch(kernel_dtype(x), x.data_ptr(), bias.data_ptr(),
                             (size_t)rows, (int)x.size(1), current_stream());
}

// the same, and p = max_pool2d(x, 2, 2)
static void conv_bias_relu_pool_(at::Tensor x, at::Tensor bias,
                                 at::Tensor p) {
  check_epi_act(x, "x");
  check_epi_bias(bias, x, "bias");
  check_epi_pooled(p, x, "p");
  bagua_epi_bias_relu_pool_launch(
      kernel_dtype(x), x.data_ptr(), bias.data_ptr(), p.data_ptr(),
      (size_t)(p.size(0) * p.size(2) * p.size(3)), (int)p.size(3),
      (int)x.size(1), current_stream());
}

// f32 [blocks, C] scratch of the bias-gradient reduction; from torch's
// allocator, so a captured graph keeps it
static at::Tensor epi_partial(const at::Tensor& y, int64_t work_rows) {
  const int64_t blocks = (int64_t)bagua_epi_partial_rows(
      kernel_dtype(y), (size_t)work_rows, (int)y.size(1));
  return at::empty({blocks, y.size(1)}, y.options().dtype(at::kFloat));
}

// dx = y <= 0 ? 0 : g; db = sum of dx over N, H, W when given
static void conv_relu_bwd(at::Tensor g, at::Tensor y, at::Tensor dx,
                          std::optional<at::Tensor> db) {
  const int64_t rows = check_epi_act(y, "y");
  check_epi_like(g, y, "g");
  check_epi_like(dx, y, "dx");
  at::Tensor partial;
  if (db.has_value()) {
    check_epi_bias(*db, y, "db");
    partial = epi_partial(y, rows);
  }
  bagua_epi_relu_bwd_launch(
      kernel_dtype(y), g.data_ptr(), y.data_ptr(), dx.data_ptr(),
      db.has_value() ? (float*)partial.data_ptr() : nullptr,
      db.has_value() ? db->data_ptr() : nullptr, (size_t)rows,
      (int)y.size(1), current_stream());
}

// g at pooled size: the gradient goes to each window's winner in y
static void conv_pool_relu_bwd(at::Tensor g, at::Tensor y, at::Tensor dx,
                               std::optional<at::Tensor> db) {
  check_epi_act(y, "y");
  check_epi_pooled(g, y, "g");
  check_epi_like(dx, y, "dx");
  const int64_t orows = g.size(0) * g.size(2) * g.size(3);
  at::Tensor partial;
  if (db.has_value()) {
    check_epi_bias(*db, y, "db");
    partial = epi_partial(y, orows);
  }
  bagua_epi_pool_relu_bwd_launch(
      kernel_dtype(y), g.data_ptr(), y.data_ptr(), dx.data_ptr(),
      db.has_value() ? (float*)partial.data_ptr() : nullptr,
      db.has_value() ? db->data_ptr() : nullptr, (size_t)orows,
      (int)g.size(3), (int)y.size(1), current_stream());
}

// ---------------------------------------------------------------------------
// first convolution (first_conv_kernels.hip): Conv2d(3, 64, 3, padding=1)
// with bias and ReLU on a channels-last bf16 image
// ---------------------------------------------------------------------------

// the image; returns its pixel count N*H*W
static int64_t check_first_conv_x(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda(), "x must be a GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 3 &&
                  x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "x must be (N, 3, H, W) and channels-last contiguous");
  const int64_t rows = x.size(0) * x.size(2) * x.size(3);
  TORCH_CHECK(rows > 0 && rows < kInt31,
              "x: N*H*W must be at least 1 and below 2^31");
  return rows;
}

// the (64, 3, 3, 3) weight or its gradient: dense, in either memory format
static void check_first_conv_weight(const at::Tensor& w,
                                    const at::Tensor& x, const char* what) {
  TORCH_CHECK(w.is_cuda() && w.device() == x.device() &&
                  w.scalar_type() == at::kBFloat16,
              what, " must be bf16 on x's device");
  TORCH_CHECK(w.dim() == 4 && w.size(0) == 64 && w.size(1) == 3 &&
                  w.size(2) == 3 && w.size(3) == 3,
              what, " must be (64, 3, 3, 3)");
  TORCH_CHECK(w.is_contiguous() ||
                  w.is_contiguous(at::MemoryFormat::ChannelsLast),
              what, " must be contiguous or channels-last contiguous");
}

// the 64-channel activation of the stage, or its gradient
static void check_first_conv_act(const at::Tensor& t, const at::Tensor& x,
                                 const char* what) {
  check_epi_act(t, what);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.device() == x.device() &&
                  t.size(0) == x.size(0) && t.size(1) == 64 &&
                  t.size(2) == x.size(2) && t.size(3) == x.size(3),
              what, " must be (N, 64, H, W) bf16 on x's device");
}

// y = relu(conv2d(x, weight, padding=1) + bias)
static at::Tensor first_conv_bias_relu(at::Tensor x, at::Tensor weight,
                                       at::Tensor bias) {
  check_first_conv_x(x);
  check_first_conv_weight(weight, x, "weight");
  at::Tensor y = at::empty({x.size(0), 64, x.size(2), x.size(3)},
                           x.options().memory_format(
                               at::MemoryFormat::ChannelsLast));
  check_first_conv_act(y, x, "y");
  check_epi_bias(bias, y, "bias");
  const long ws[4] = {(long)weight.stride(0), (long)weight.stride(1),
                      (long)weight.stride(2), (long)weight.stride(3)};
  bagua_first_conv_fwd_launch(x.data_ptr(), weight.data_ptr(), ws,
                              bias.data_ptr(), y.data_ptr(), (int)x.size(0),
                              (int)x.size(2), (int)x.size(3),
                              current_stream());
  return y;
}

// dx = y <= 0 ? 0 : g is formed on the fly; returns the weight gradient, in
// weight_like's strides, and the bias gradient
static std::tuple<at::Tensor, at::Tensor> first_conv_bias_relu_bwd(
    at::Tensor g, at::Tensor y, at::Tensor x, at::Tensor weight_like) {
  check_first_conv_x(x);
  check_first_conv_weight(weight_like, x, "weight_like");
  check_first_conv_act(y, x, "y");
  check_first_conv_act(g, x, "g");
  at::Tensor dw = at::empty_strided(weight_like.sizes(),
                                    weight_like.strides(), y.options());
  at::Tensor db = at::empty({64}, y.options());
  const int N = (int)x.size(0), H = (int)x.size(2), W = (int)x.size(3);
  // f32 [blocks, 64 * 28] partial sums; from torch's allocator, so a
  // captured graph keeps it
  at::Tensor partial = at::empty(
      {(int64_t)bagua_first_conv_partial_rows(N, H, W),
       (int64_t)bagua_first_conv_partial_cols()},
      y.options().dtype(at::kFloat));
  const long ws[4] = {(long)dw.stride(0), (long)dw.stride(1),
                      (long)dw.stride(2), (long)dw.stride(3)};
  bagua_first_conv_bwd_launch(g.data_ptr(), y.data_ptr(), x.data_ptr(),
                              (float*)partial.data_ptr(), dw.data_ptr(), ws,
                              db.data_ptr(), N, H, W, current_stream());
  return std::make_tuple(dw, db);
}

static py::bytes nccl_unique_id() {
  ncclUniqueId id;
  NCCL_CHECK(ncclGetUniqueId(&id));
  return py::bytes((const char*)&id, sizeof(id));
}


// ---------------------------------------------------------------------------
// C ABI for non-Python hosts (reference: bagua-core-c/src/lib.rs:23-347).
// Raw-pointer variants of the communicator surface; dtype codes:
// 0=f32 1=f16 2=bf16 3=u8 4=i64. op codes = bagua_amd.ReduceOp values.
// ---------------------------------------------------------------------------

namespace {
ncclDataType_t c_dtype(int d) {
  switch (d) {
    case 0: return ncclFloat32;
    case 1: return ncclFloat16;
    case 2: return ncclBfloat16;
    case 3: return ncclUint8;
    case 4: return ncclInt64;
    default: return ncclFloat32;
  }
}
}  // namespace

extern "C" {

void* bagua_comm_create(int rank, int nranks, int device,
                        uintptr_t stream, const char* uid_bytes,
                        size_t uid_len) {
  try {
    return new Communicator(rank, nranks, device, stream,
                            std::string(uid_bytes, uid_len));
  } catch (...) {
    return nullptr;
  }
}

void bagua_comm_destroy(void* comm) {
  delete (Communicator*)comm;
}

int bagua_comm_rank(void* comm) { return ((Communicator*)comm)->rank(); }
int bagua_comm_nranks(void* comm) {
  return ((Communicator*)comm)->nranks();
}
void bagua_comm_abort(void* comm) { ((Communicator*)comm)->abort(); }

int bagua_comm_allreduce_inplace(void* comm, void* ptr, size_t numel,
                                 int dtype, int op, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  if (c->nranks() == 1) return 0;
  return ncclAllReduce(ptr, ptr, numel, c_dtype(dtype), nccl_op(op),
                       c->raw(), (hipStream_t)stream) == ncclSuccess
             ? 0 : -1;
}

int bagua_comm_broadcast(void* comm, void* ptr, size_t numel, int dtype,
                         int src, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  if (c->nranks() == 1) return 0;
  return ncclBroadcast(ptr, ptr, numel, c_dtype(dtype), src, c->raw(),
                       (hipStream_t)stream) == ncclSuccess ? 0 : -1;
}

int bagua_comm_allgather_inplace(void* comm, void* ptr, size_t numel,
                                 int dtype, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  if (c->nranks() == 1) return 0;
  size_t chunk = numel / c->nranks();
  size_t es = dtype == 3 ? 1 : (dtype == 1 || dtype == 2) ? 2
              : dtype == 4 ? 8 : 4;
  char* own = (char*)ptr + c->rank() * chunk * es;
  return ncclAllGather(own, ptr, chunk, c_dtype(dtype), c->raw(),
                       (hipStream_t)stream) == ncclSuccess ? 0 : -1;
}

int bagua_nccl_unique_id(char* out, size_t cap) {
  if (cap < sizeof(ncclUniqueId)) return -1;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return -1;
  std::memcpy(out, &id, sizeof(id));
  return (int)sizeof(id);
}

// --- full collective mirror for non-Python hosts (reference:
// bagua-core-c/src/lib.rs:23-347 exposed the whole communicator surface;
// dtype codes: 0=f32 1=f16 2=bf16 3=u8 4=i64) -------------------------

static size_t c_esize(int dtype) {
  switch (dtype) {
    case 3: return 1;
    case 1: case 2: return 2;
    case 4: return 8;
    default: return 4;
  }
}

int bagua_comm_reduce_inplace(void* comm, void* ptr, size_t numel,
                              int dtype, int dst, int op,
                              uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  if (c->nranks() == 1) return 0;
  return ncclReduce(ptr, ptr, numel, c_dtype(dtype), nccl_op(op), dst,
                    c->raw(), (hipStream_t)stream) == ncclSuccess ? 0 : -1;
}

int bagua_comm_reduce_scatter_inplace(void* comm, void* ptr, size_t numel,
                                      int dtype, int op, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  if (c->nranks() == 1) return 0;
  if (numel % c->nranks() != 0) return -2;
  size_t chunk = numel / c->nranks();
  char* own = (char*)ptr + c->rank() * chunk * c_esize(dtype);
  return ncclReduceScatter(ptr, own, chunk, c_dtype(dtype), nccl_op(op),
                           c->raw(), (hipStream_t)stream) == ncclSuccess
             ? 0 : -1;
}

int bagua_comm_alltoall(void* comm, const void* send, void* recv,
                        size_t numel, int dtype, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  if (c->nranks() == 1) {
    return hipMemcpyAsync(recv, send, numel * c_esize(dtype),
                          hipMemcpyDeviceToDevice,
                          (hipStream_t)stream) == hipSuccess ? 0 : -1;
  }
  if (numel % c->nranks() != 0) return -2;
  return ncclAllToAll(send, recv, numel / c->nranks(), c_dtype(dtype),
                      c->raw(), (hipStream_t)stream) == ncclSuccess
             ? 0 : -1;
}

int bagua_comm_send(void* comm, const void* ptr, size_t numel, int dtype,
                    int dst, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  return ncclSend(ptr, numel, c_dtype(dtype), dst, c->raw(),
                  (hipStream_t)stream) == ncclSuccess ? 0 : -1;
}

int bagua_comm_recv(void* comm, void* ptr, size_t numel, int dtype,
                    int src, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  return ncclRecv(ptr, numel, c_dtype(dtype), src, c->raw(),
                  (hipStream_t)stream) == ncclSuccess ? 0 : -1;
}

int bagua_comm_gather(void* comm, const void* send, void* recv,
                      size_t numel, int dtype, int dst, uintptr_t stream) {
  // grouped p2p gather: every rank sends its chunk to dst
  Communicator* c = (Communicator*)comm;
  size_t es = c_esize(dtype);
  if (ncclGroupStart() != ncclSuccess) return -1;
  if (c->rank() == dst) {
    for (int r = 0; r < c->nranks(); ++r) {
      if (ncclRecv((char*)recv + (size_t)r * numel * es, numel,
                   c_dtype(dtype), r, c->raw(),
                   (hipStream_t)stream) != ncclSuccess)
        return -1;
    }
  }
  if (ncclSend(send, numel, c_dtype(dtype), dst, c->raw(),
               (hipStream_t)stream) != ncclSuccess)
    return -1;
  return ncclGroupEnd() == ncclSuccess ? 0 : -1;
}

int bagua_comm_scatter(void* comm, const void* send, void* recv,
                       size_t numel, int dtype, int src, uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  size_t es = c_esize(dtype);
  if (ncclGroupStart() != ncclSuccess) return -1;
  if (c->rank() == src) {
    for (int r = 0; r < c->nranks(); ++r) {
      if (ncclSend((const char*)send + (size_t)r * numel * es, numel,
                   c_dtype(dtype), r, c->raw(),
                   (hipStream_t)stream) != ncclSuccess)
        return -1;
    }
  }
  if (ncclRecv(recv, numel, c_dtype(dtype), src, c->raw(),
               (hipStream_t)stream) != ncclSuccess)
    return -1;
  return ncclGroupEnd() == ncclSuccess ? 0 : -1;
}

int bagua_comm_group_start(void) {
  return ncclGroupStart() == ncclSuccess ? 0 : -1;
}

int bagua_comm_group_end(void) {
  return ncclGroupEnd() == ncclSuccess ? 0 : -1;
}

// barrier = 1-element allreduce (reference: communication.py:1377-1401),
// followed by a stream sync so the host really is past it
int bagua_comm_barrier(void* comm, void* scratch_one_elem,
                       uintptr_t stream) {
  Communicator* c = (Communicator*)comm;
  if (c->nranks() > 1) {
    if (ncclAllReduce(scratch_one_elem, scratch_one_elem, 1, ncclFloat32,
                      ncclSum, c->raw(),
                      (hipStream_t)stream) != ncclSuccess)
      return -1;
  }
  return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? 0 : -1;
}

}  // extern "C"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "bagua_amd native core (RCCL over xGMI + CDNA4 kernels)";

  py::class_<Communicator, std::shared_ptr<Communicator>>(m, "Communicator")
      .def(py::init<int, int, int, uintptr_t, const std::string&>())
      .def("rank", &Communicator::rank)
      .def("nranks", &Communicator::nranks)
      .def("abort", &Communicator::abort)
      .def("destroy", &Communicator::destroy)
      .def("group_start", &Communicator::group_start)
      .def("group_end", &Communicator::group_end)
      .def("allreduce_inplace", &Communicator::allreduce_inplace)
      .def("allreduce", &Communicator::allreduce)
      .def("reduce_inplace", &Communicator::reduce_inplace)
      .def("broadcast", &Communicator::broadcast)
      .def("allgather", &Communicator::allgather)
      .def("allgather_inplace", &Communicator::allgather_inplace)
      .def("reduce_scatter", &Communicator::reduce_scatter)
      .def("reduce_scatter_inplace", &Communicator::reduce_scatter_inplace)
      .def("alltoall", &Communicator::alltoall)
      .def("alltoall_inplace", &Communicator::alltoall_inplace)
      .def("alltoall_v", &Communicator::alltoall_v)
      .def("send", &Communicator::send)
      .def("recv", &Communicator::recv)
      .def("gather", &Communicator::gather)
      .def("gather_inplace", &Communicator::gather_inplace)
      .def("scatter", &Communicator::scatter)
      .def("scatter_inplace", &Communicator::scatter_inplace);

  py::class_<BucketExecutor>(m, "BucketExecutor")
      .def(py::init<std::shared_ptr<Communicator>,
                    std::shared_ptr<Communicator>,
                    std::shared_ptr<Communicator>, uintptr_t>(),
           py::arg("global_comm"), py::arg("intra_comm") = nullptr,
           py::arg("inter_comm") = nullptr, py::arg("stream") = 0)
      .def("register_bucket", &BucketExecutor::register_bucket)
      .def("execute", &BucketExecutor::execute)
      .def("wait_pending", &BucketExecutor::wait_pending)
      .def("synchronize", &BucketExecutor::synchronize)
      .def("clear_buckets", &BucketExecutor::clear_buckets);

  py::class_<P2PAlltoAll>(m, "P2PAlltoAll")
      .def(py::init<int, int, uintptr_t, int64_t>(), py::arg("rank"),
           py::arg("nranks"), py::arg("stream"), py::arg("capacity"))
      .def("handles", &P2PAlltoAll::handles)
      .def("connect", &P2PAlltoAll::connect)
      .def("capacity", &P2PAlltoAll::capacity)
      .def("alltoall", &P2PAlltoAll::alltoall)
      .def("allgather_inplace", &P2PAlltoAll::allgather_inplace);

  m.def("nccl_unique_id", &nccl_unique_id);
  m.def("average_inplace", &average_inplace);
  m.def("add_inplace", &add_inplace);
  m.def("substract_inplace", &substract_inplace);
  m.def("addmul_inplace", &addmul_inplace);
  m.def("divide_inplace", &divide_inplace);
  m.def("async_model_average", &async_model_average);
  m.def("reduce_chunk_inplace", &reduce_chunk_inplace);
  m.def("compress_chunked", &compress_chunked);
  m.def("decompress_chunked", &decompress_chunked);
  m.def("dequant_reduce", &dequant_reduce);
  m.def("compressed_chunk_stride", &compressed_chunk_stride);
  m.def("fused_sgd_step", &fused_sgd_step);
  m.def("fused_sgd_mixed_step", &fused_sgd_mixed_step);
  m.def("fused_adam_step", &fused_adam_step);
  m.def("fused_sgd_step_segments", &fused_sgd_step_segments, py::arg("p"),
        py::arg("grads"), py::arg("offsets"), py::arg("m"), py::arg("lr"),
        py::arg("momentum"), py::arg("dampening"), py::arg("weight_decay"),
        py::arg("nesterov"), py::arg("momentum_initialized"));
  m.def("fused_sgd_mixed_step_segments", &fused_sgd_mixed_step_segments,
        py::arg("p"), py::arg("grads"), py::arg("offsets"),
        py::arg("master"), py::arg("m"), py::arg("lr"), py::arg("momentum"),
        py::arg("dampening"), py::arg("weight_decay"), py::arg("nesterov"),
        py::arg("momentum_initialized"));
  m.def("fused_adam_step_segments", &fused_adam_step_segments, py::arg("p"),
        py::arg("grads"), py::arg("offsets"), py::arg("m"), py::arg("v"),
        py::arg("step"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("weight_decay"), py::arg("adamw"));
  m.def("moe_assign_slots", &moe_assign_slots, py::arg("expert"),
        py::arg("num_experts"), py::arg("capacity"), py::arg("base"),
        py::arg("slot"), py::arg("counts"), py::arg("src"));
  m.def("moe_gather_rows", &moe_gather_rows, py::arg("x"), py::arg("src"),
        py::arg("out"), py::arg("w") = py::none(),
        py::arg("dest") = py::none());
  m.def("moe_combine_rows", &moe_combine_rows, py::arg("eo"),
        py::arg("dest"), py::arg("out"), py::arg("w") = py::none());
  m.def("moe_row_dot", &moe_row_dot);
  m.def("conv_bias_relu_", &conv_bias_relu_, py::arg("x"), py::arg("bias"));
  m.def("conv_bias_relu_pool_", &conv_bias_relu_pool_, py::arg("x"),
        py::arg("bias"), py::arg("p"));
  m.def("conv_relu_bwd", &conv_relu_bwd, py::arg("g"), py::arg("y"),
        py::arg("dx"), py::arg("db") = py::none());
  m.def("conv_pool_relu_bwd", &conv_pool_relu_bwd, py::arg("g"),
        py::arg("y"), py::arg("dx"), py::arg("db") = py::none());
  m.def("first_conv_bias_relu", &first_conv_bias_relu, py::arg("x"),
        py::arg("weight"), py::arg("bias"));
  m.def("first_conv_bias_relu_bwd", &first_conv_bias_relu_bwd, py::arg("g"),
        py::arg("y"), py::arg("x"), py::arg("weight_like"));
}
