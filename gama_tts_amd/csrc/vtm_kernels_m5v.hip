// The voice variant of the reference model 5 kernel (vtm5_synth_kernel with kVoices5Flag: gvtm_synthesize_voices_* on a
// gvtm_plan_create_model5_voices plan).  It has a translation unit, and so a code object, of its own: the code object of
// vtm_kernels.hip keeps exactly the kernels it had, byte for byte, the single-voice model 5 kernels among them.
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

hipError_t launch_synth5_voices(const SynthArgs& args, size_t groups, hipStream_t stream)
{
	return launch_synth5_shape<false, 0, true>(args, groups, stream);
}

} // namespace gvtm
