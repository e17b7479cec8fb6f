// kv_radam_ops_hip.cc — TensorFlow custom op KvVariableGroupSparseApplyRectifiedAdam over libkvhip.so (include/kvhip.h
// kv_apply_group_rectified_adam).  Built into the same plug-in as kv_variable_ops_hip.cc (INTEGRATION.md has the build
// line): the KvVariable resources those ops create are the ones this op reads.  The schema is the reference's
// (tfplus/kv_variable/ops/training_ops.cc:1194-1217: name, inputs and their order, attrs and defaults);
// tests/test_group_radam.py checks it against tests/golden/tf_reference_radam_ops.json.  DEVICE_GPU kernels only (a
// TensorFlow-ROCm build): tensor.data() goes straight to the C ABI on TF's stream; the resources and every scalar — the
// three bool inputs included — in host memory, grad and indices on the device.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "kvhip.h"
#include "unique_input.h"
#include "tensorflow/core/framework/common_shape_fns.h"
#include "tensorflow/core/framework/node_def.pb.h"
#include "tensorflow/core/framework/op.h"
#include "tensorflow/core/framework/op_kernel.h"
#include "tensorflow/core/framework/resource_mgr.h"
#include "tensorflow/core/framework/shape_inference.h"
#include "tensorflow/core/util/gpu_kernel_helper.h"

namespace tfplus_hip {
using namespace tensorflow;  // NOLINT
using shape_inference::InferenceContext;

static Status FromKv(int rc) {
  if (rc == KV_OK) return OkStatus();
  return Status(static_cast<tsl::error::Code>(rc), kv_last_error());
}
static Status FromHip(hipError_t e, const char* what) {
  if (e == hipSuccess) return OkStatus();
  return errors::Internal(what, ": ", hipGetErrorString(e));
}
#define HIP_RET(expr)                                 \
  do {                                                \
    Status _s = FromHip((expr), #expr);               \
    if (!_s.ok()) return _s;                          \
  } while (0)

// ---- the resource class of kv_variable_ops_hip.cc --------------------------------------------------------------------
// One class across the two translation units of the plug-in: the definitions below are token for token those of
// kv_variable_ops_hip.cc (tests/test_group_radam.py compares them), as the one-definition rule requires of a class that
// LookupResource finds by its type.
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

static Status KeyTypeMatches(const KvHipResource* r, const Tensor& ids) {
  const DataType t = ids.dtype();
  const bool ok = (r->key_dtype() == DT_INT32 && t == DT_INT32) ||
                  (r->key_dtype() != DT_INT32 && (t == DT_INT64 || t == DT_UINT64));
  if (!ok) return errors::InvalidArgument("indices dtype ", DataTypeString(t), " does not match the table's key dtype ",
                                          DataTypeString(r->key_dtype()));
  return OkStatus();
}

// array_ops.unique's output 0 feeds `indices`: the one-launch apply (kv_apply_*_unique), as kv_variable_ops_hip.cc decides it
static bool IndicesComeFromUnique(const NodeDef& def, int input) {
  const char* e = std::getenv("TFPLUS_KV_UNIQUE_INDICES");
  if (e && e[0] == '0') return false;
  if (e && e[0] == '1') return true;
  if (input >= def.input_size()) return false;
  return kv_shim::InputIsUniqueValues(def.input(input));
}

static hipStream_t TfStream(OpKernelContext* ctx) { return GetGpuStream(ctx); }

// ---- KvVariableGroupSparseApplyRectifiedAdam : ops/training_ops.cc:1194-1217, kernels/training_ops.cc:6694-6978 -------
REGISTER_OP("KvVariableGroupSparseApplyRectifiedAdam")
    .Input("var: resource")
    .Input("opt: resource")
    .Input("grad: T")
    .Input("indices: Tindices")
    .Input("lr: T")
    .Input("beta1_power: T")
    .Input("beta2_power: T")
    .Input("beat1: T")
    .Input("beta2: T")
    .Input("epsilon: T")
    .Input("l1: T")
    .Input("l2: T")
    .Input("l21: T")
    .Input("r_t: T")
    .Input("tractable: bool")
    .Input("amsgrad: bool")
    .Input("use_nesterov: bool")
    .Attr("T: numbertype")
    .Attr("Tindices: {int32, int64, uint64, string}")
    .Attr("use_locking: bool = false")
    .SetShapeFn(shape_inference::NoOutputs);

// kv_apply_group_rectified_adam[_unique|_tok]; the call rule of the other optimizer ops: the forward
// lookup's token when these are its ids, else the one-launch form when `indices` comes from array_ops.unique, else plain
class KvGroupRadamGpuOp : public OpKernel {
 public:
  explicit KvGroupRadamGpuOp(OpKernelConstruction* c) : OpKernel(c), unique_(IndicesComeFromUnique(c->def(), 3)) {}
  void Compute(OpKernelContext* ctx) override {
    KvHipResource *var = nullptr, *opt = nullptr;
    OP_REQUIRES_OK(ctx, LookupResource(ctx, HandleFromInput(ctx, 0), &var));
    core::ScopedUnref unref_var(var);
    OP_REQUIRES_OK(ctx, LookupResource(ctx, HandleFromInput(ctx, 1), &opt));
    core::ScopedUnref unref_opt(opt);
    for (int i = 4; i <= 16; ++i)
      OP_REQUIRES(ctx, TensorShapeUtils::IsScalar(ctx->input(i).shape()),
                  errors::InvalidArgument("input ", i, " is not a scalar: ", ctx->input(i).shape().DebugString()));
    auto f = [&](int i) { return ctx->input(i).scalar<float>()(); };          // host memory (registration below)
    auto b = [&](int i) { return ctx->input(i).scalar<bool>()() ? 1 : 0; };   // tractable, amsgrad, use_nesterov
    const Tensor& grad = ctx->input(2);
    const Tensor& ids = ctx->input(3);
    OP_REQUIRES(ctx, TensorShapeUtils::IsVector(ids.shape()), errors::InvalidArgument("indices must be one-dimensional"));
    OP_REQUIRES_OK(ctx, KeyTypeMatches(var, ids));
    OP_REQUIRES(ctx, grad.dims() >= 1 && grad.dim_size(0) == ids.dim_size(0),
                errors::InvalidArgument("grad must be the same size as indices in the first dimension."));
    OP_REQUIRES(ctx, grad.NumElements() == ids.dim_size(0) * var->dim(),
                errors::InvalidArgument("var and grad must match in dimension 1"));
    std::lock_guard<std::mutex> l(*var->mu());
    const int64_t n = ids.dim_size(0);
    // the forward lookup's batch token when these are its very ids (same buffer and length, kept alive by token_keep)
    const kv_batch_token_t token = (var->token != 0 && var->token_n == n && var->token_ids == ids.data()) ? var->token : 0;
    var->token = 0;   // one apply per lookup: a second optimizer op on the same ids rebuilds the index
    var->token_keep = Tensor();
    if (n == 0) return;
    const float* g = static_cast<const float*>(grad.data());
    if (token == 0 && unique_)
      OP_REQUIRES_OK(ctx, FromKv(kv_apply_group_rectified_adam_unique(var->h(), opt->h(), g, ids.data(), n, f(4), f(5), f(6), f(7),
                                                                      f(8), f(9), f(10), f(11), f(12), f(13), b(14), b(15), b(16),
                                                                      TfStream(ctx))));
    else
      OP_REQUIRES_OK(ctx, FromKv(kv_apply_group_rectified_adam_tok(var->h(), opt->h(), g, ids.data(), n, f(4), f(5), f(6), f(7),
                                                                   f(8), f(9), f(10), f(11), f(12), f(13), b(14), b(15), b(16),
                                                                   token, TfStream(ctx))));
  }

 private:
  const bool unique_;
};
#define KV_GPU_RADAM_HOST .HostMemory("var").HostMemory("opt").HostMemory("lr").HostMemory("beta1_power")                    \
      .HostMemory("beta2_power").HostMemory("beat1").HostMemory("beta2").HostMemory("epsilon").HostMemory("l1")            \
      .HostMemory("l2").HostMemory("l21").HostMemory("r_t").HostMemory("tractable").HostMemory("amsgrad")                  \
      .HostMemory("use_nesterov")
#define KV_REGISTER_RADAM_GPU(NAME, CLASS)                                                                                  \
  REGISTER_KERNEL_BUILDER(Name(NAME).Device(DEVICE_GPU) KV_GPU_RADAM_HOST.TypeConstraint<float>("T").TypeConstraint<int32>("Tindices"), CLASS);   \
  REGISTER_KERNEL_BUILDER(Name(NAME).Device(DEVICE_GPU) KV_GPU_RADAM_HOST.TypeConstraint<float>("T").TypeConstraint<int64_t>("Tindices"), CLASS); \
  REGISTER_KERNEL_BUILDER(Name(NAME).Device(DEVICE_GPU) KV_GPU_RADAM_HOST.TypeConstraint<float>("T").TypeConstraint<uint64>("Tindices"), CLASS)
KV_REGISTER_RADAM_GPU("KvVariableGroupSparseApplyRectifiedAdam", KvGroupRadamGpuOp);

}  // namespace tfplus_hip
