// The voice variant of the float class of the reference model 5 kernel (vtm5_synth_kernel with kFloat5Flag and
// kVoices5Flag: gvtm_synthesize_voices_* on a gvtm_plan_create_model5_float_voices plan), in both shapes of the float class.
// A translation unit, and so a code object, of its own: the code objects of vtm_kernels.hip, vtm_kernels_m5v.hip and
// vtm_kernels_m5f.hip keep exactly the kernels they had.  Compiled with -ffp-contract=off (Makefile), as vtm_kernels_m5f.hip
// is: the float class rounds every product before it adds.
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

hipError_t launch_synth5_float_voices(const SynthArgs& args, size_t groups, int index, hipStream_t stream)
{
	if (!args.row_map || !args.group_voice || !args.k5const) return hipErrorInvalidValue;
	return index == 1 ? launch_synth5_shape<true, 1, true>(args, groups, stream) : launch_synth5_shape<true, 0, true>(args, groups, stream);
}

} // namespace gvtm
