// The targets variant of the synthesis kernel under several voices (vtm_synth_kernel with kVoicesFlag and kTargetsFlag:
// gvtm_synthesize_targets_voices_device) in every shape of one, two and four rows the voices launch can pick.  A translation
// unit, and so a code object, of its own: the code objects of vtm_kernels.hip and vtm_kernels_targets.hip keep exactly the
// kernels they had, and the three compile side by side.  The shapes and their launch are vtm_kernel_shapes.hpp's, the one
// table and the one launch_v2: this unit is one launch_v2_variant<kVoicesFlag | kTargetsFlag> call.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "vtm_design.hpp"
#include "vtm_kernels.hpp"
#include "vtm_math.hpp"
#include "vtm_targets.hpp"

namespace gvtm {

namespace {
#include "vtm_device_common.inc"
} // namespace

#include "vtm_kernel_v2.inc"
#include "vtm_kernel_shapes.hpp"

hipError_t launch_synth_targets_voices(const SynthArgs& args, size_t groups, int precision, int rows, hipStream_t stream)
{
	return launch_v2_variant<v2::kVoicesFlag | v2::kTargetsFlag>(args, groups, precision, rows, stream);
}

} // namespace gvtm
