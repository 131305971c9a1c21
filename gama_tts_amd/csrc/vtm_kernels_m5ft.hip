// The targets variant of the reference model 5 kernel in the float class (vtm5_synth_kernel with kFloat5Flag and
// kTargets5Flag: VocalTractModel5<float,1>(config, interactive = true) fed parameter targets,
// gvtm_synthesize_targets_model5_device and gvtm_stream_push_targets_model5 on a gvtm_plan_create_model5_float plan), in both
// of its shapes.  A code object of its
// own; compiled with -ffp-contract=off as vtm_kernels_m5f.hip is (Makefile): the float class rounds every product before it
// adds, and the division by f0 is one rounding of its own.
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

hipError_t launch_synth5_float_targets(const SynthArgs& args, size_t batch, int index, hipStream_t stream)
{
	if (!synth5_targets_args(args)) return hipErrorInvalidValue;
	return index == 1 ? launch_synth5_shape<true, 1, false, true>(args, batch, stream) : launch_synth5_shape<true, 0, false, true>(args, batch, stream);
}

} // namespace gvtm
