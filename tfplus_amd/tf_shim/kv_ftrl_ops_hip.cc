// kv_ftrl_ops_hip.cc — TensorFlow custom ops KvVariableSparseApplyFtrlV2 and KvVariableGroupSparseApplyFtrlV2 over
// libkvhip.so (include/kvhip.h kv_apply_ftrl_v2 / kv_apply_group_ftrl_v2).  Built into the same plug-in as
// kv_variable_ops_hip.cc (INTEGRATION.md has the build line): the KvVariable resources those ops create are the ones
// these ops read — the resource class lives in kv_shim_common.h, which every unit of the plug-in includes.  Schemas are
// the reference's (tfplus/kv_variable/ops/training_ops.cc:103-133: names, inputs and their order, attrs and defaults);
// tests/test_ftrl_v2.py checks them against tests/golden/tf_reference_ftrl_ops.json.
// DEVICE_GPU kernels only (a TensorFlow-ROCm build): tensor.data() goes straight to the C ABI on TF's stream, the
// resources and the scalar hyper-parameters in host memory, grad and indices on the device.
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

// ---- KvVariableSparseApplyFtrlV2 : ops/training_ops.cc:103-117, kernels/training_ops.cc:281-526 -----------------------
REGISTER_OP("KvVariableSparseApplyFtrlV2")
    .Input("var: resource")
    .Input("accum: resource")
    .Input("linear: resource")
    .Input("grad: T")
    .Input("indices: Tindices")
    .Input("lr: T")
    .Input("l1: T")
    .Input("l2: T")
    .Input("l2_shrinkage: T")
    .Input("lr_power: T")
    .Attr("T: numbertype")
    .Attr("Tindices: {int32, int64, uint64, string}")
    .Attr("use_locking: bool = false")
    .SetShapeFn(shape_inference::NoOutputs);

// ---- KvVariableGroupSparseApplyFtrlV2 : ops/training_ops.cc:119-133, kernels/training_ops.cc:805-1059 -----------------
REGISTER_OP("KvVariableGroupSparseApplyFtrlV2")
    .Input("var: resource")
    .Input("accum: resource")
    .Input("linear: resource")
    .Input("grad: T")
    .Input("indices: Tindices")
    .Input("lr: T")
    .Input("l1: T")
    .Input("l2: T")
    .Input("l2_shrinkage: T")
    .Input("lr_power: T")
    .Attr("T: numbertype")
    .Attr("Tindices: {int32, int64, uint64, string}")
    .Attr("use_locking: bool = false")
    .SetShapeFn(shape_inference::NoOutputs);

// GROUP = 0: kv_apply_ftrl_v2[_unique|_tok]; 1: kv_apply_group_ftrl_v2[_unique|_tok]
constexpr ApplyInputs kFtrlV2Inputs = {3, 3, 4, 5, 9};
template <int GROUP>
static int CallFtrlV2(OpKernelContext* ctx, const kv_handle_t* h, const float* grad, const void* ids, int64_t n,
                      const kv_batch_token_t* token, hipStream_t st) {
  auto f = [&](int i) { return ctx->input(i).scalar<float>()(); };   // host memory (registration below)
  if (!token)
    return (GROUP ? kv_apply_group_ftrl_v2_unique : kv_apply_ftrl_v2_unique)(h[0], h[1], h[2], grad, ids, n, f(5), f(6), f(7),
                                                                             f(8), f(9), st);
  return (GROUP ? kv_apply_group_ftrl_v2_tok : kv_apply_ftrl_v2_tok)(h[0], h[1], h[2], grad, ids, n, f(5), f(6), f(7), f(8), f(9),
                                                                     *token, st);
}

template <int GROUP>
class KvFtrlV2GpuOp : public OpKernel {
 public:
  explicit KvFtrlV2GpuOp(OpKernelConstruction* c)
      : OpKernel(c), unique_(IndicesComeFromUnique(c->def(), kFtrlV2Inputs.indices)) {}
  void Compute(OpKernelContext* ctx) override {
    OP_REQUIRES_OK(ctx, ApplyOnDevice(ctx, kFtrlV2Inputs, unique_,
                                      [ctx](auto... a) { return CallFtrlV2<GROUP>(ctx, a...); }));
  }

 private:
  const bool unique_;
};
#define KV_GPU_FTRL_V2_HOST .HostMemory("var").HostMemory("accum").HostMemory("linear").HostMemory("lr").HostMemory("l1")  \
      .HostMemory("l2").HostMemory("l2_shrinkage").HostMemory("lr_power")
#define KV_REGISTER_FTRL_V2_GPU(NAME, CLASS)                                                                                \
  REGISTER_KERNEL_BUILDER(Name(NAME).Device(DEVICE_GPU) KV_GPU_FTRL_V2_HOST.TypeConstraint<float>("T").TypeConstraint<int32>("Tindices"), CLASS);   \
  REGISTER_KERNEL_BUILDER(Name(NAME).Device(DEVICE_GPU) KV_GPU_FTRL_V2_HOST.TypeConstraint<float>("T").TypeConstraint<int64_t>("Tindices"), CLASS); \
  REGISTER_KERNEL_BUILDER(Name(NAME).Device(DEVICE_GPU) KV_GPU_FTRL_V2_HOST.TypeConstraint<float>("T").TypeConstraint<uint64>("Tindices"), CLASS)
KV_REGISTER_FTRL_V2_GPU("KvVariableSparseApplyFtrlV2", KvFtrlV2GpuOp<0>);
KV_REGISTER_FTRL_V2_GPU("KvVariableGroupSparseApplyFtrlV2", KvFtrlV2GpuOp<1>);

}  // namespace tfplus_hip
