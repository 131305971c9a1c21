// The targets variant of the synthesis kernel (vtm_synth_kernel with kTargetsFlag: gvtm_synthesize_targets_device) in every
// single-voice shape of one, two and four rows, and the check kernel that runs in front of it.  A translation unit, and so a
// code object, of its own: the code object of vtm_kernels.hip keeps exactly the kernels it had, and the two compile side by
// side.  The shapes and their launch are vtm_kernel_shapes.hpp's, the one table and the one launch_v2: this unit is its
// check kernel and one launch_v2_variant<kTargetsFlag> call.
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
	return launch_v2_variant<v2::kTargetsFlag>(args, batch, precision, rows, stream);
}

hipError_t launch_targets_check(const TargetsCheckArgs& args, hipStream_t stream)
{
	if (args.batch == 0) return hipSuccess;
	hipLaunchKernelGGL(vtm_targets_check_kernel, dim3(static_cast<unsigned>(args.batch)), dim3(64), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
