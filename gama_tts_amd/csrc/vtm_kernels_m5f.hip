// The float class of the reference model 5 kernel (vtm5_synth_kernel with kFloat5Flag: VocalTractModel5<float,1>, plans of
// gvtm_plan_create_model5_float).  A translation unit, and so a code object, of its own, as the voice variant has: the
// code object of vtm_kernels.hip keeps exactly the kernels it had.  Compiled with -ffp-contract=off (Makefile): the float
// class rounds every product before it adds, and bit identity with it leaves no room for a fused multiply-add.
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

size_t synth5_float_lds_bytes(int index)
{
	return index == 1 ? m5_lds_bytes<true, 1>() : m5_lds_bytes<true, 0>();
}

hipError_t launch_synth5_float(const SynthArgs& args, size_t batch, int index, hipStream_t stream)
{
	if (args.row_map || !args.k5const) return hipErrorInvalidValue; // (one voice per plan)
	return index == 1 ? launch_synth5_shape<true, 1>(args, batch, stream) : launch_synth5_shape<true, 0>(args, batch, stream);
}

} // namespace gvtm
