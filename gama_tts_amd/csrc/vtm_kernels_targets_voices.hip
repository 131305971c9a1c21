// The targets variant of the synthesis kernel under several voices (vtm_synth_kernel with kVoicesFlag and kTargetsFlag:
// gvtm_synthesize_targets_voices_device) in every shape of one, two and four rows the voices launch can pick.  A translation
// unit, and so a code object, of its own: the code objects of vtm_kernels.hip and vtm_kernels_targets.hip keep exactly the
// kernels they had, and the three compile side by side.  The shapes are vtm_kernel_shapes.hpp's, the one table.
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

namespace {

// launch_v2 of vtm_kernels.hip for the voice variant from targets: the same checks of the ring (args.xr: the longest of the
// launch's voices), the same LDS, one workgroup per group of the row map
template <typename S>
hipError_t launch_v2_targets_voices(const SynthArgs& args, size_t groups, hipStream_t stream)
{
	if constexpr (S::U == 8) {
		// the product's shapes only (eight rows are a diagnostics build's forced shape)
		return hipErrorInvalidValue;
	} else {
		auto fn = v2::vtm_synth_kernel<typename S::CT, typename S::ST, S::D, S::U, S::C, S::NH, S::LAYOUT | v2::kVoicesFlag | v2::kTargetsFlag>;
		if (args.xr < ring_length(args.k, S::C) || (args.xr & (args.xr - 1)) != 0 || 2 * S::C + 4 * args.k.pad + 64 > args.xr) return hipErrorInvalidValue;
		if (!args.k.upsampling && args.xr != kSrcRing) return hipErrorInvalidValue;
		static_assert(!v2::float_arg_consts<typename S::CT, S::D, S::U, true>(), "several voices: each voice's constants come from its block in LDS");
		const size_t lds = S::lds_bytes(args.xr);
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(groups)), dim3(S::kWaves * 64), lds, stream, args);
		return hipGetLastError();
	}
}

} // namespace

hipError_t launch_synth_targets_voices(const SynthArgs& args, size_t groups, int precision, int rows, hipStream_t stream)
{
	if (!args.row_map || !args.group_voice || !args.tg_offsets || !args.tg_steps || !args.tg_values || !args.frame_counts || !args.tg_voice_N || !args.tg_voice_invN) {
		return hipErrorInvalidValue;
	}
	return with_shape(precision, rows, args.k.section_delay, args.k.layout, hipErrorInvalidValue,
			[&](auto s) { return launch_v2_targets_voices<decltype(s)>(args, groups, stream); });
}

} // namespace gvtm
