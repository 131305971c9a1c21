// The targets variant of the reference model 5 kernel in the double class (vtm5_synth_kernel with kTargets5Flag:
// VocalTractModel5<double,1>(config, interactive = true) fed parameter targets, gvtm_synthesize_targets_model5_device and
// gvtm_stream_push_targets_model5 on a gvtm_plan_create_model5 plan), in both of its shapes: one utterance per workgroup and two.  A translation unit, and so a
// code object, of its own, as the voice variant and the float class have: the code object of vtm_kernels.hip keeps exactly
// the kernels it had.  Plain flags, as vtm_kernels.hip has them: the same kernel text gives the same samples in each, and the
// targets filter's additions keep their order by the pragma of vtm_targets.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "vtm_design.hpp"
#include "vtm_kernels.hpp"
#include "vtm_math.hpp"

namespace gvtm {

namespace {
#include "vtm_device_common.inc"
} // namespace

#include "vtm_kernel_v2.inc"
#include "vtm_kernel_m5.inc"

hipError_t launch_synth5_targets(const SynthArgs& args, size_t batch, int index, hipStream_t stream)
{
	if (!synth5_targets_args(args)) return hipErrorInvalidValue;
	return index == 1 ? launch_synth5_shape<false, 1, false, true>(args, batch, stream) : launch_synth5_shape<false, 0, false, true>(args, batch, stream);
}

} // namespace gvtm
