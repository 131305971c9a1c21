// Parameter-modification gestures applied to frames (vtm_modification.hpp; ParameterModificationSynthesis.cpp:117-194): the
// host's restatement and the device's two kernels, one code object built without FMA contraction.
//
// Two kernels, one wavefront per utterance, no scratch:
//   copy      the utterance's statuses -- lanes stride over its gestures and points -- then the base row leaves as 16-byte
//             units, 64 consecutive units per store instruction (as integers: every bit of a NaN stays), and lane 0 writes
//             the frame count (0 for a refused utterance, whose row is untouched) and the status.  HBM-bound: 64 bytes per
//             frame read (a shared base mostly from cache) and written.
//   gestures  lane g walks gesture g (hence GVTM_MAX_GESTURES = 64).  Every gesture reads the base row, so the in-order rule
//             is: on one parameter the frames from a later gesture's first frame on are that gesture's.  A lane therefore
//             neither writes nor walks past `stop`, the smallest first frame among the later gestures on its parameter: no
//             two lanes store to one address, and what is stored is what the gestures one after the other would leave.
//             Bound by the walk: a lane is one chain of two dependent double additions per internal step, N steps per point
//             with the walk's jump, and the frames' 4-byte loads and stores at a 64-byte stride hide behind it.
// The second kernel reads the first one's frame counts: an utterance it left 0 is skipped.
#include "vtm_modification.hpp"

namespace gvtm {

int32_t modification_apply(int64_t cs, int64_t N, const float* frames, size_t n_frames, const int32_t* gestures, const int64_t* gesture_offsets,
		size_t n_gestures, const int32_t* point_steps, const float* point_values, float* frames_out)
{
	if (n_frames < 2) return kModificationNoBase;
	if (n_gestures > GVTM_MAX_GESTURES) return kModificationTooMany;
	for (size_t g = 0; g < n_gestures; ++g) {
		if (modification_bad_gesture(gestures[2 * g], gestures[2 * g + 1])) return kModificationBadGesture;
	}
	const int64_t first = n_gestures ? gesture_offsets[0] : 0, end = n_gestures ? gesture_offsets[n_gestures] : 0;
	for (int64_t j = first; j < end; ++j) {
		if (!modification_finite(point_values[j])) return kModificationBadGesture;
	}
	for (size_t g = 0; g < n_gestures; ++g) {
		for (int64_t j = gesture_offsets[g]; j < gesture_offsets[g + 1]; ++j) {
			if (point_steps[j] < 0 || (j > gesture_offsets[g] && point_steps[j] <= point_steps[j - 1])) return kModificationBadSteps;
		}
	}
	for (size_t i = 0; i < n_frames * GVTM_N_PARAM; ++i) frames_out[i] = frames[i];
	for (size_t g = 0; g < n_gestures; ++g) {
		const int64_t p0 = gesture_offsets[g];
		modification_gesture(frames, frames_out, static_cast<int64_t>(n_frames), cs, N, gestures[2 * g], gestures[2 * g + 1], point_steps + p0,
				point_values + p0, gesture_offsets[g + 1] - p0, static_cast<int64_t>(n_frames));
	}
	return kModificationOk;
}

namespace {

constexpr int kMaxGestures = GVTM_MAX_GESTURES;
static_assert(kMaxGestures == 64, "one lane of the wavefront per gesture");

// what both kernels read of an utterance's tables
struct Utterance {
	int32_t status;
	int64_t base;       // its base row
	int32_t voice;
	int64_t n_frames;
	int64_t first_gesture;
	int n_gestures;
};

// One wavefront, all 64 lanes active, the same answer in every lane: status 1 and 2 as far as the tables alone tell them
__device__ __forceinline__ Utterance utterance_of(const ModificationArgs& a, size_t utt)
{
	Utterance u{};
	u.status = kModificationNoBase;
	u.base = a.base_ids ? static_cast<int64_t>(a.base_ids[utt]) : static_cast<int64_t>(utt);
	u.voice = a.voice_ids ? a.voice_ids[utt] : 0;
	if (u.base < 0 || u.base >= a.n_bases || u.voice < 0 || u.voice >= a.n_voices) return u;
	u.n_frames = a.base_frame_counts[u.base];
	if (u.n_frames < 2 || u.n_frames > static_cast<int64_t>(a.max_frames)) return u;
	u.status = kModificationTooMany;
	u.first_gesture = a.utt_gestures[utt];
	const int64_t n = a.utt_gestures[utt + 1] - u.first_gesture;
	if (u.first_gesture < 0 || n < 0 || n > kMaxGestures) return u; // (a negative offset counts as one that decreases)
	u.n_gestures = static_cast<int>(n);
	u.status = kModificationOk;
	return u;
}

__global__ __launch_bounds__(64) void vtm_modification_copy_kernel(const ModificationArgs a)
{
	const size_t utt = blockIdx.x;
	const int lane = threadIdx.x;
	Utterance u = utterance_of(a, utt);
	if (u.status == kModificationOk) {
		// lane g: gesture g's offsets and its (parameter, operation)
		const bool mine = lane < u.n_gestures;
		int64_t p0 = 0, p1 = 0;
		bool bad = false;
		if (mine) {
			p0 = a.gesture_offsets[u.first_gesture + lane];
			p1 = a.gesture_offsets[u.first_gesture + lane + 1];
		}
		if (__ballot(mine && (p0 < 0 || p1 < p0))) {
			u.status = kModificationTooMany;
		} else {
			if (mine) bad = modification_bad_gesture(a.gestures[2 * (u.first_gesture + lane)], a.gestures[2 * (u.first_gesture + lane) + 1]);
			// every point of the utterance, 64 at a time: its value
			const int64_t first = u.n_gestures ? a.gesture_offsets[u.first_gesture] : 0;
			const int64_t end = u.n_gestures ? a.gesture_offsets[u.first_gesture + u.n_gestures] : 0;
			for (int64_t j = first + lane; j < end; j += 64) bad = bad || !modification_finite(a.point_values[j]);
			if (__ballot(bad)) {
				u.status = kModificationBadGesture;
			} else {
				// ... and, gesture by gesture, its step against the one before
				for (int g = 0; g < u.n_gestures; ++g) {
					const int64_t g0 = __shfl(p0, g), g1 = __shfl(p1, g);
					for (int64_t j = g0 + lane; j < g1; j += 64) {
						const int32_t step = a.point_steps[j];
						bad = bad || step < 0 || (j > g0 && step <= a.point_steps[j - 1]);
					}
				}
				if (__ballot(bad)) u.status = kModificationBadSteps;
			}
		}
	}
	if (u.status == kModificationOk) {
		const uint4* __restrict__ in = reinterpret_cast<const uint4*>(a.base_params) + u.base * static_cast<int64_t>(a.max_frames) * 4;
		uint4* __restrict__ out = reinterpret_cast<uint4*>(a.params_out) + static_cast<int64_t>(utt) * static_cast<int64_t>(a.max_frames) * 4;
		const int64_t units = u.n_frames * 4; // a frame is four 16-byte units
		for (int64_t i = lane; i < units; i += 64) out[i] = in[i];
	}
	if (lane == 0) {
		a.frame_counts_out[utt] = u.status == kModificationOk ? static_cast<int32_t>(u.n_frames) : 0;
		if (a.status) a.status[utt] = u.status;
	}
}

__global__ __launch_bounds__(64) void vtm_modification_gestures_kernel(const ModificationArgs a)
{
#pragma clang fp contract(off)
	// per gesture its parameter and its first frame (n_frames and beyond: it never acts)
	__shared__ int parameter[kMaxGestures];
	__shared__ int64_t first_frame[kMaxGestures];
	const size_t utt = blockIdx.x;
	const int lane = threadIdx.x;
	if (a.frame_counts_out[utt] == 0) return; // refused by the copy kernel (which left every good utterance 2 frames or more)
	const Utterance u = utterance_of(a, utt);
	if (u.status != kModificationOk || u.n_gestures == 0) return;
	const int64_t cs = a.kconst[u.voice].control_steps;
	const int64_t N = modification_filter_length(a.k5const ? a.k5const[u.voice].sample_rate : static_cast<double>(a.kconst[u.voice].sample_rate));
	const bool mine = lane < u.n_gestures;
	int p = -1, op = 0;
	int64_t p0 = 0, n_points = 0, first = u.n_frames;
	if (mine) {
		const int64_t g = u.first_gesture + lane;
		p = a.gestures[2 * g];
		op = a.gestures[2 * g + 1];
		p0 = a.gesture_offsets[g];
		n_points = a.gesture_offsets[g + 1] - p0;
		if (n_points > 0) {
			const int64_t f = modification_first_frame(a.point_steps[p0], cs);
			first = f < u.n_frames ? f : u.n_frames;
		}
	}
	parameter[lane] = p;
	first_frame[lane] = first;
	__syncthreads();
	if (!mine || first >= u.n_frames) return;
	int64_t stop = u.n_frames;
	for (int g = lane + 1; g < u.n_gestures; ++g) {
		if (parameter[g] == p && first_frame[g] < stop) stop = first_frame[g];
	}
	if (stop <= first) return;
	const float* orig = a.base_params + u.base * static_cast<int64_t>(a.max_frames) * GVTM_N_PARAM;
	float* out = a.params_out + static_cast<int64_t>(utt) * static_cast<int64_t>(a.max_frames) * GVTM_N_PARAM;
	modification_gesture(orig, out, u.n_frames, cs, N, p, op, a.point_steps + p0, a.point_values + p0, n_points, stop);
}

} // namespace

hipError_t launch_apply_modifications(const ModificationArgs& args, hipStream_t stream)
{
	if (args.batch == 0) return hipSuccess;
	const dim3 per_utterance(static_cast<unsigned>(args.batch));
	hipLaunchKernelGGL(vtm_modification_copy_kernel, per_utterance, dim3(64), 0, stream, args);
	hipLaunchKernelGGL(vtm_modification_gestures_kernel, per_utterance, dim3(64), 0, stream, args);
	return hipGetLastError();
}

} // namespace gvtm
