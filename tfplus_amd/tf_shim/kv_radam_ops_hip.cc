// kv_radam_ops_hip.cc — TensorFlow custom op KvVariableGroupSparseApplyRectifiedAdam over libkvhip.so (include/kvhip.h
// kv_apply_group_rectified_adam).  Built into the same plug-in as kv_variable_ops_hip.cc (INTEGRATION.md has the build
// line): the KvVariable resources those ops create are the ones this op reads — the resource class lives in
// kv_shim_common.h, which every unit of the plug-in includes.  The schema is the reference's
// (tfplus/kv_variable/ops/training_ops.cc:1194-1217: name, inputs and their order, attrs and defaults);
// tests/test_group_radam.py checks it against tests/golden/tf_reference_radam_ops.json.  DEVICE_GPU kernels only (a
// TensorFlow-ROCm build): tensor.data() goes straight to the C ABI on TF's stream; the resources and every scalar — the
// three bool inputs included — in host memory, grad and indices on the device.
#include <hip/hip_runtime.h>

#include "kv_shim_common.h"   // KvHipResource (the one definition all units of the plug-in share), ApplyOnDevice
#include "kvhip.h"
#include "tensorflow/core/framework/common_shape_fns.h"
#include "tensorflow/core/framework/node_def.pb.h"
#include "tensorflow/core/framework/op.h"
#include "tensorflow/core/framework/op_kernel.h"
#include "tensorflow/core/framework/resource_mgr.h"
#include "tensorflow/core/framework/shape_inference.h"

namespace tfplus_hip {
using namespace tensorflow;  // NOLINT
using shape_inference::InferenceContext;

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
constexpr ApplyInputs kGroupRadamInputs = {2, 2, 3, 4, 16};
static int CallGroupRadam(OpKernelContext* ctx, const kv_handle_t* h, const float* grad, const void* ids, int64_t n,
                          const kv_batch_token_t* token, hipStream_t st) {
  auto f = [&](int i) { return ctx->input(i).scalar<float>()(); };          // host memory (registration below)
  auto b = [&](int i) { return ctx->input(i).scalar<bool>()() ? 1 : 0; };   // tractable, amsgrad, use_nesterov
  if (!token)
    return kv_apply_group_rectified_adam_unique(h[0], h[1], grad, ids, n, f(4), f(5), f(6), f(7), f(8), f(9), f(10), f(11), f(12),
                                                f(13), b(14), b(15), b(16), st);
  return kv_apply_group_rectified_adam_tok(h[0], h[1], grad, ids, n, f(4), f(5), f(6), f(7), f(8), f(9), f(10), f(11), f(12),
                                           f(13), b(14), b(15), b(16), *token, st);
}

class KvGroupRadamGpuOp : public OpKernel {
 public:
  explicit KvGroupRadamGpuOp(OpKernelConstruction* c)
      : OpKernel(c), unique_(IndicesComeFromUnique(c->def(), kGroupRadamInputs.indices)) {}
  void Compute(OpKernelContext* ctx) override {
    OP_REQUIRES_OK(ctx, ApplyOnDevice(ctx, kGroupRadamInputs, unique_,
                                      [ctx](auto... a) { return CallGroupRadam(ctx, a...); }));
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
