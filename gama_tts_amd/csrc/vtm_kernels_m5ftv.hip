// The targets variant of the reference model 5 kernel under several voices, in the float class (vtm5_synth_kernel with
// kFloat5Flag, kTargets5Flag and kVoices5Flag: gvtm_synthesize_targets_model5_voices_device and a stream's
// gvtm_stream_push_targets_model5_voices on a gvtm_plan_create_model5_float_voices plan), in both targets shapes of the float class.  A code object of its own: those of
// vtm_kernels_m5fv.hip and vtm_kernels_m5ft.hip keep exactly the kernels they had.  Compiled with -ffp-contract=off as they
// are (Makefile): the float class rounds every product before it adds, and the division by f0 is one rounding of its own.
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

hipError_t launch_synth5_float_targets_voices(const SynthArgs& args, size_t groups, int index, hipStream_t stream)
{
	if (!synth5_targets_voices_args(args)) return hipErrorInvalidValue;
	return index == 1 ? launch_synth5_shape<true, 1, true, true>(args, groups, stream) : launch_synth5_shape<true, 0, true, true>(args, groups, stream);
}

} // namespace gvtm
