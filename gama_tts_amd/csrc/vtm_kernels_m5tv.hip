// The targets variant of the reference model 5 kernel under several voices, in the double class (vtm5_synth_kernel with
// kTargets5Flag and kVoices5Flag: gvtm_synthesize_targets_model5_voices_device and a stream's
// gvtm_stream_push_targets_model5_voices on a gvtm_plan_create_model5_voices plan), in
// the one-utterance shape, the only one the voice variant has.  A translation unit, and so a code object, of its own: the
// code objects of vtm_kernels.hip, vtm_kernels_m5v.hip and vtm_kernels_m5t.hip keep exactly the kernels they had.  Plain
// flags, as vtm_kernels_m5t.hip and vtm_kernels_m5v.hip have them: the same kernel text gives the same samples in each, and
// the targets filter's additions keep their order by the pragma of vtm_targets.hpp.
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

hipError_t launch_synth5_targets_voices(const SynthArgs& args, size_t groups, hipStream_t stream)
{
	if (!synth5_targets_voices_args(args)) return hipErrorInvalidValue;
	return launch_synth5_shape<false, 0, true, true>(args, groups, stream);
}

} // namespace gvtm
