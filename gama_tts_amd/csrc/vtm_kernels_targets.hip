// The targets variant of the synthesis kernel (vtm_synth_kernel with kTargetsFlag: gvtm_synthesize_targets_device) in every
// single-voice shape of one, two and four rows, and the check kernel that runs in front of it.  A translation unit, and so a
// code object, of its own: the code object of vtm_kernels.hip keeps exactly the kernels it had, and the two compile side by
// side.  The shapes are vtm_kernel_shapes.hpp's, the one table.
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

// launch_v2 of vtm_kernels.hip for the targets variant: the same checks of the ring, the same LDS, one workgroup per S::U utterances
template <typename S>
hipError_t launch_v2_targets(const SynthArgs& args, size_t batch, hipStream_t stream)
{
	if constexpr (S::U == 8) {
		// the product's shapes only (eight rows are a diagnostics build's forced shape)
		return hipErrorInvalidValue;
	} else {
		auto fn = v2::vtm_synth_kernel<typename S::CT, typename S::ST, S::D, S::U, S::C, S::NH, S::LAYOUT | v2::kTargetsFlag>;
		if (args.xr < ring_length(args.k, S::C) || (args.xr & (args.xr - 1)) != 0 || 2 * S::C + 4 * args.k.pad + 64 > args.xr) return hipErrorInvalidValue;
		if (!args.k.upsampling && args.xr != kSrcRing) return hipErrorInvalidValue;
		if constexpr (v2::float_arg_consts<typename S::CT, S::D, S::U, false>()) {
			if (args.fir_k.f[kFirKConsts + kKfBasicIncrement] != static_cast<float>(args.k.basic_increment)) return hipErrorInvalidValue;
		}
		const size_t lds = S::lds_bytes(args.xr);
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
		if (e != hipSuccess) return e;
		const unsigned groups = static_cast<unsigned>((batch + S::U - 1) / S::U);
		hipLaunchKernelGGL(fn, dim3(groups), dim3(S::kWaves * 64), lds, stream, args);
		return hipGetLastError();
	}
}

// One wavefront per utterance, all 64 lanes active until the store: lanes 0 .. 15 hold the utterance's 16 lists, then all
// lanes stride over each list's points; every verdict is a ballot, so every lane holds the same status.  The first status
// that applies, every point being looked at for 3 before any for 4 (gama_vtm.h).
__global__ __launch_bounds__(64) void vtm_targets_check_kernel(const TargetsCheckArgs a)
{
	const size_t utt = blockIdx.x;
	const int lane = threadIdx.x;
	const int64_t steps = a.step_counts ? static_cast<int64_t>(a.step_counts[utt]) : static_cast<int64_t>(a.max_steps);
	const bool mine = lane < GVTM_N_PARAM;
	int32_t status = kTargetsOk;
	int64_t list = 0, p0 = 0, p1 = 0;
	if (mine) list = a.list_ids ? static_cast<int64_t>(a.list_ids[utt * GVTM_N_PARAM + lane]) : static_cast<int64_t>(utt * GVTM_N_PARAM + lane);
	if (a.voice_ids && (a.voice_ids[utt] < 0 || a.voice_ids[utt] >= a.n_voices)) {
		status = kTargetsBadVoice;
	} else if (steps < 0 || steps > static_cast<int64_t>(a.max_steps) || __ballot(mine && (list < 0 || list >= a.n_lists))) {
		status = kTargetsBadCount;
	} else {
		if (mine) {
			p0 = a.list_offsets[list];
			p1 = a.list_offsets[list + 1];
		}
		if (__ballot(mine && (p0 < 0 || p1 < p0))) {
			status = kTargetsBadOffsets;
		} else {
			bool bad = false;
			for (int p = 0; p < GVTM_N_PARAM; ++p) {
				const int64_t g0 = __shfl(p0, p), g1 = __shfl(p1, p);
				for (int64_t j = g0 + lane; j < g1; j += 64) bad = bad || !modification_finite(a.point_values[j]);
			}
			if (__ballot(bad)) {
				status = kTargetsBadValue;
			} else {
				for (int p = 0; p < GVTM_N_PARAM; ++p) {
					const int64_t g0 = __shfl(p0, p), g1 = __shfl(p1, p);
					for (int64_t j = g0 + lane; j < g1; j += 64) bad = bad || targets_bad_step(a.point_steps, g0, j);
				}
				if (__ballot(bad)) status = kTargetsBadSteps;
			}
		}
	}
	if (lane == 0) {
		a.steps_out[utt] = status == kTargetsOk ? static_cast<int32_t>(steps) : 0;
		if (a.status) a.status[utt] = status;
	}
}

} // namespace

hipError_t launch_synth_targets(const SynthArgs& args, size_t batch, int precision, int rows, hipStream_t stream)
{
	// (a stream's launch, args.stream, takes the shapes launch_v2 gives a stream of frames: the ring is the stream's, args.xr)
	if (!args.tg_offsets || !args.tg_steps || !args.tg_values || !args.frame_counts || args.row_map || args.tg_N < 1) return hipErrorInvalidValue;
	return with_shape(precision, rows, args.k.section_delay, args.k.layout, hipErrorInvalidValue,
			[&](auto s) { return launch_v2_targets<decltype(s)>(args, batch, stream); });
}

hipError_t launch_targets_check(const TargetsCheckArgs& args, hipStream_t stream)
{
	if (args.batch == 0) return hipSuccess;
	hipLaunchKernelGGL(vtm_targets_check_kernel, dim3(static_cast<unsigned>(args.batch)), dim3(64), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
