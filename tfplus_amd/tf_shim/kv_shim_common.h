// kv_shim_common.h — what the translation units of the TensorFlow plug-in share: the status helpers, the KvVariable
// resource class (ONE definition: LookupResource finds a resource by its type, so kv_variable_ops_hip.cc, which creates
// the resources, and kv_ftrl_ops_hip.cc / kv_radam_ops_hip.cc, which read them, must all see this very class), the checks
// of an optimizer op's grad and indices, and the one sequence every optimizer kernel runs (ApplyOnDevice, ApplyStaged).
// Found next to the .cc files, like unique_input.h.
#ifndef TFPLUS_AMD_TF_SHIM_KV_SHIM_COMMON_H_
#define TFPLUS_AMD_TF_SHIM_KV_SHIM_COMMON_H_
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "kvhip.h"
#include "unique_input.h"
#include "tensorflow/core/framework/node_def.pb.h"
#include "tensorflow/core/framework/op_kernel.h"
#include "tensorflow/core/framework/resource_mgr.h"
#include "tensorflow/core/util/gpu_kernel_helper.h"   // GetGpuStream: gpuStream_t is hipStream_t under TENSORFLOW_USE_ROCM

namespace tfplus_hip {
using namespace tensorflow;  // NOLINT

inline Status FromKv(int rc) {
  if (rc == KV_OK) return OkStatus();
  return Status(static_cast<tsl::error::Code>(rc), kv_last_error());
}
inline Status FromHip(hipError_t e, const char* what) {
  if (e == hipSuccess) return OkStatus();
  return errors::Internal(what, ": ", hipGetErrorString(e));
}
#define HIP_OK(ctx, expr) OP_REQUIRES_OK(ctx, FromHip((expr), #expr))
#define HIP_RET(expr)                                 \
  do {                                                \
    Status _s = FromHip((expr), #expr);               \
    if (!_s.ok()) return _s;                          \
  } while (0)

// Ring of pinned host + device staging buffers.  A slot is reused only after the stream has passed the event
// recorded behind its last use; buffers grow geometrically and are never freed before the resource dies.
class StagingRing {
 public:
  struct Slot {
    char* host = nullptr;
    char* dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
  };
  ~StagingRing() {
    for (Slot& s : slots_) {
      if (s.done) { hipEventSynchronize(s.done); hipEventDestroy(s.done); }
      if (s.host) hipHostFree(s.host);
      if (s.dev) hipFree(s.dev);
    }
  }
  // a slot with room for `bytes` on both sides (waits for the slot's previous user)
  Status Acquire(size_t bytes, Slot** out) {
    Slot& s = slots_[cursor_++ % kSlots];
    if (s.done) HIP_RET(hipEventSynchronize(s.done));
    if (s.cap < bytes) {
      size_t cap = s.cap ? s.cap : (1u << 20);
      while (cap < bytes) cap *= 2;
      char *h = nullptr, *d = nullptr;
      HIP_RET(hipHostMalloc(reinterpret_cast<void**>(&h), cap));
      hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), cap);
      if (e != hipSuccess) { hipHostFree(h); return FromHip(e, "hipMalloc(staging)"); }
      if (s.host) hipHostFree(s.host);
      if (s.dev) hipFree(s.dev);
      s.host = h; s.dev = d; s.cap = cap;
    }
    if (!s.done) HIP_RET(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    *out = &s;
    return OkStatus();
  }
  // host tensor -> device (asynchronous; the slot stays busy until Release)
  static Status Upload(Slot* s, const void* src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return OkStatus();
    std::memcpy(s->host, src, bytes);
    HIP_RET(hipMemcpyAsync(s->dev, s->host, bytes, hipMemcpyHostToDevice, st));
    return OkStatus();
  }
  // device -> host tensor (synchronous: the op's output must be complete when Compute returns)
  static Status Download(Slot* s, void* dst, size_t bytes, hipStream_t st) {
    if (bytes == 0) return OkStatus();
    HIP_RET(hipMemcpyAsync(s->host, s->dev, bytes, hipMemcpyDeviceToHost, st));
    HIP_RET(hipStreamSynchronize(st));
    std::memcpy(dst, s->host, bytes);
    return OkStatus();
  }
  static Status Release(Slot* s, hipStream_t st) { return FromHip(hipEventRecord(s->done, st), "hipEventRecord"); }

 private:
  static constexpr int kSlots = 6;
  Slot slots_[kSlots];
  unsigned cursor_ = 0;
};

// The resource the handle points at: owns one kv_handle_t, its stream and its staging ring.
class KvHipResource : public ResourceBase {
 public:
  KvHipResource(kv_handle_t h, int dim, DataType key_dtype) : h_(h), dim_(dim), key_dtype_(key_dtype) {
    hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking);
  }
  ~KvHipResource() override {
    if (stream_) hipStreamSynchronize(stream_);
    kv_destroy(h_);
    if (stream_) kv_forget_stream(stream_);   // an optimizer op on this stream left it as the slot tables' last one
    if (stream_) hipStreamDestroy(stream_);
  }
  string DebugString() const override { return "KvHipResource"; }
  kv_handle_t h() const { return h_; }
  int dim() const { return dim_; }
  DataType key_dtype() const { return key_dtype_; }
  hipStream_t stream() const { return stream_; }
  StagingRing* ring() { return &ring_; }
  std::mutex* mu() { return &mu_; }
  // the batch a training lookup left behind (kv_gather_or_insert_tok): token + what identified the ids
  kv_batch_token_t token = 0;
  const void* token_ids = nullptr;
  int64_t token_n = 0;
  uint64_t token_sum = 0;
  Tensor token_keep;   // DEVICE_GPU: a reference to the lookup's ids tensor, held until the token is used or dropped — while
                       // it is held the allocator cannot hand the buffer to another tensor, so "same address and length"
                       // means "same tensor" (BFC readily reuses a freed buffer of the same size)
  // the init table as the graph gave it (KvVariableExport returns it: dynamic_save.hpp:110-118)
  std::vector<float> init_host;
  int64_t init_rows = 0;

 private:
  kv_handle_t h_;
  int dim_;
  DataType key_dtype_;
  hipStream_t stream_ = nullptr;
  StagingRing ring_;
  std::mutex mu_;   // one Compute at a time moves data through this resource's ring
};

// every kernel starts the same way
#define KV_RESOURCE(ctx, index, var)                                          \
  KvHipResource* var = nullptr;                                               \
  OP_REQUIRES_OK(ctx, LookupResource(ctx, HandleFromInput(ctx, index), &var)); \
  core::ScopedUnref unref_##var(var)

// content fingerprint of an ids tensor: EVERY byte takes part (the token is only passed on when the optimizer op
// receives the very ids the lookup saw — kvhip.h promises a right result only then; a sampled hash would let two
// batches that differ in an unsampled id share an index).  The ids are on the host here and about to be copied
// anyway; one multiply-xor per 8 bytes is nothing next to the PCIe transfer.  TF-core's de-duplicated indices
// never match and take the general path.
inline uint64_t Fingerprint(const void* p, size_t bytes) {
  const unsigned char* c = static_cast<const unsigned char*>(p);
  uint64_t h = 1469598103934665603ull ^ bytes;
  size_t i = 0;
  for (; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, c + i, 8);
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  for (; i < bytes; ++i) h = (h ^ c[i]) * 1099511628211ull;
  return h;
}

inline Status KeyTypeMatches(const KvHipResource* r, const Tensor& ids) {
  const DataType t = ids.dtype();
  const bool ok = (r->key_dtype() == DT_INT32 && t == DT_INT32) ||
                  (r->key_dtype() != DT_INT32 && (t == DT_INT64 || t == DT_UINT64));
  if (!ok) return errors::InvalidArgument("indices dtype ", DataTypeString(t), " does not match the table's key dtype ",
                                          DataTypeString(r->key_dtype()));
  return OkStatus();
}

// Are the `indices` of this optimizer node unique?  In an UNCHANGED reference graph they are: the processor patch
// (python/ops/variable_scope.py:1096-1106) sends the gradient through TF-core's _deduplicate_indexed_slices, whose
// array_ops.unique produces the node ".../Unique" whose output 0 feeds input `input` here.  Then the op is ONE launch
// (kv_apply_*_unique, include/kvhip.h).  The test is the producer's name and output slot (unique_input.h: the exact leaf
// Unique / UniqueV2 with TensorFlow's _<n> suffix, slot 0 only — ":1" is the inverse index vector) — a heuristic; the
// promise it makes is also guarded on the device (an id listed twice raises the table's error word: the next op on the
// table fails with InvalidArgument).  TFPLUS_KV_UNIQUE_INDICES=0 never takes that path, =1 always does.
inline bool IndicesComeFromUnique(const NodeDef& def, int input) {
  const char* e = std::getenv("TFPLUS_KV_UNIQUE_INDICES");
  if (e && e[0] == '0') return false;
  if (e && e[0] == '1') return true;
  if (input >= def.input_size()) return false;
  return kv_shim::InputIsUniqueValues(def.input(input));
}

// TF's own compute stream of a DEVICE_GPU kernel
inline hipStream_t TfStream(OpKernelContext* ctx) { return GetGpuStream(ctx); }

// ---- grad and indices of an optimizer op --------------------------------------------------------------------------------
inline Status CheckGradIds(const KvHipResource* var, const Tensor& grad, const Tensor& ids) {
  if (!TensorShapeUtils::IsVector(ids.shape())) return errors::InvalidArgument("indices must be one-dimensional");
  TF_RETURN_IF_ERROR(KeyTypeMatches(var, ids));
  if (grad.dims() < 1 || grad.dim_size(0) != ids.dim_size(0))
    return errors::InvalidArgument("grad must be the same size as indices in the first dimension.");
  if (grad.NumElements() != ids.dim_size(0) * var->dim())
    return errors::InvalidArgument("var and grad must match in dimension 1");
  return OkStatus();
}

// DEVICE_CPU: gradient + indices on the var's ring; the var's stream carries the whole op.  (The slot resources' own
// streams must see the work the var's stream was given, and vice versa: the C ABI orders ops of one table across streams
// itself (kvhip.h), so nothing to do here beyond using var's stream.)
struct GradIds {
  StagingRing::Slot *sg = nullptr, *si = nullptr;
  int64_t n = 0;
  kv_batch_token_t token = 0;
};
inline Status StageGradIds(OpKernelContext* ctx, KvHipResource* var, const Tensor& grad, const Tensor& ids, GradIds* g) {
  TF_RETURN_IF_ERROR(CheckGradIds(var, grad, ids));
  g->n = ids.dim_size(0);
  if (g->n == 0) return OkStatus();
  TF_RETURN_IF_ERROR(var->ring()->Acquire(grad.TotalBytes(), &g->sg));
  TF_RETURN_IF_ERROR(var->ring()->Acquire(ids.TotalBytes(), &g->si));
  TF_RETURN_IF_ERROR(StagingRing::Upload(g->sg, grad.data(), grad.TotalBytes(), var->stream()));
  TF_RETURN_IF_ERROR(StagingRing::Upload(g->si, ids.data(), ids.TotalBytes(), var->stream()));
  // the batch token of the forward lookup, when these are the very ids it saw (same length and content); TF-core's
  // _deduplicate_indexed_slices hands over unique ids, which never match: those take the general path
  if (var->token != 0 && var->token_n == g->n && var->token_sum == Fingerprint(ids.data(), ids.TotalBytes()))
    g->token = var->token;
  return OkStatus();
}
inline Status ReleaseGradIds(KvHipResource* var, GradIds* g) {
  if (g->sg) TF_RETURN_IF_ERROR(StagingRing::Release(g->sg, var->stream()));
  if (g->si) TF_RETURN_IF_ERROR(StagingRing::Release(g->si, var->stream()));
  return OkStatus();
}

// DEVICE_GPU: gradient + indices device-resident: shape checks, and the lookup's token when these are its very ids (same
// buffer and length, kept alive by token_keep)
inline Status DeviceGradIds(KvHipResource* var, const Tensor& grad, const Tensor& ids, int64_t* n, kv_batch_token_t* token) {
  TF_RETURN_IF_ERROR(CheckGradIds(var, grad, ids));
  *n = ids.dim_size(0);
  *token = (var->token != 0 && var->token_n == *n && var->token_ids == ids.data()) ? var->token : 0;
  var->token = 0;   // one apply per lookup: a second optimizer op on the same ids rebuilds the index
  var->token_keep = Tensor();
  return OkStatus();
}

// ---- the one sequence of an optimizer kernel ----------------------------------------------------------------------------
// Where an optimizer op has its inputs: the var and its slot tables are inputs 0 .. tables - 1, the host scalars are
// inputs scalar_first .. scalar_last (a lone scalar is reported by its name).
struct ApplyInputs {
  int tables, grad, indices, scalar_first, scalar_last;
  const char* lone_scalar = nullptr;
};

// the var (0) and its slot tables, looked up in input order and released when the op is done
struct ApplyTables {
  static constexpr int kMax = 3;
  KvHipResource* r[kMax] = {nullptr, nullptr, nullptr};
  kv_handle_t h[kMax] = {nullptr, nullptr, nullptr};
  ~ApplyTables() {
    for (KvHipResource* p : r)
      if (p) p->Unref();
  }
  // what is reported first: a handle that names no KvVariable, then a hyper-parameter that is no scalar
  Status Lookup(OpKernelContext* ctx, const ApplyInputs& in) {
    if (in.tables < 1 || in.tables > kMax) return errors::Internal("optimizer op with ", in.tables, " tables");
    for (int i = 0; i < in.tables; ++i) {
      TF_RETURN_IF_ERROR(LookupResource(ctx, HandleFromInput(ctx, i), &r[i]));
      h[i] = r[i]->h();
    }
    for (int i = in.scalar_first; i <= in.scalar_last; ++i) {
      const TensorShape& s = ctx->input(i).shape();
      if (TensorShapeUtils::IsScalar(s)) continue;
      if (in.lone_scalar) return errors::InvalidArgument(in.lone_scalar, " is not a scalar: ", s.DebugString());
      return errors::InvalidArgument("input ", i, " is not a scalar: ", s.DebugString());
    }
    return OkStatus();
  }
};

// Both run: look up the tables, check the scalars' shapes, take the var's mutex, check grad and indices and work out the
// token, return when there are no ids, then `call(handles, grad, ids, n, token, stream)` -> the C ABI's return code, with
// grad and ids on the device.  token == nullptr asks for the _unique form (no token from the lookup and `indices` comes
// from array_ops.unique); else the _tok form with *token, which may be 0.
//
// DEVICE_GPU: tensor.data() goes straight to the C ABI on TF's stream.
template <typename Call>
Status ApplyOnDevice(OpKernelContext* ctx, const ApplyInputs& in, bool unique, Call call) {
  ApplyTables t;
  TF_RETURN_IF_ERROR(t.Lookup(ctx, in));
  KvHipResource* var = t.r[0];
  std::lock_guard<std::mutex> l(*var->mu());
  const Tensor& grad = ctx->input(in.grad);
  const Tensor& ids = ctx->input(in.indices);
  int64_t n = 0;
  kv_batch_token_t token = 0;
  TF_RETURN_IF_ERROR(DeviceGradIds(var, grad, ids, &n, &token));
  if (n == 0) return OkStatus();
  return FromKv(call(t.h, static_cast<const float*>(grad.data()), ids.data(), n, token == 0 && unique ? nullptr : &token,
                     TfStream(ctx)));
}

// DEVICE_CPU: grad and indices cross PCIe through the var's ring, on the var's stream; nothing is staged for no ids.
template <typename Call>
Status ApplyStaged(OpKernelContext* ctx, const ApplyInputs& in, bool unique, Call call) {
  ApplyTables t;
  TF_RETURN_IF_ERROR(t.Lookup(ctx, in));
  KvHipResource* var = t.r[0];
  std::lock_guard<std::mutex> l(*var->mu());
  GradIds g;
  TF_RETURN_IF_ERROR(StageGradIds(ctx, var, ctx->input(in.grad), ctx->input(in.indices), &g));
  if (g.n == 0) return OkStatus();
  TF_RETURN_IF_ERROR(FromKv(call(t.h, reinterpret_cast<const float*>(g.sg->dev), g.si->dev, g.n,
                                 g.token == 0 && unique ? nullptr : &g.token, var->stream())));
  return ReleaseGradIds(var, &g);
}

}  // namespace tfplus_hip
#endif  // TFPLUS_AMD_TF_SHIM_KV_SHIM_COMMON_H_
