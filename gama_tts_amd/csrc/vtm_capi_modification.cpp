// C ABI of libgama_vtm.so, parameter-modification gestures: the filter length, the rule on the host, the rule for a batch on
// the device, and the one-call entry, which puts a synthesis launch behind the two apply kernels with the plan's frame
// buffer in between.
#include "vtm_host.hpp"
#include "vtm_modification.hpp"

using namespace gvtm::host;

namespace {

// The batch of a device entry as the caller gives it
struct ModificationBatch {
	const float* d_base_params;
	const int32_t* d_base_frame_counts;
	size_t n_bases;
	const int32_t* d_base_ids;
	const int32_t* d_gestures;
	const int64_t* d_gesture_offsets;
	const int64_t* d_utt_gestures;
	const int32_t* d_point_steps;
	const float* d_point_values;
	const int32_t* d_voice_ids;
};

// What the two device entries refuse before any device work, in the order the header gives, up to the alignment; GVTM_OK
// with batch == 0 is the caller's to return.  d_params_out / null_output: the apply entry's own outputs.
int check_modifications(const gvtm_plan* plan, const ModificationBatch& in, size_t batch, const float* d_params_out = nullptr, bool null_output = false)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (batch == 0) return GVTM_OK;
	if (!in.d_base_params || !in.d_base_frame_counts || !in.d_gestures || !in.d_gesture_offsets || !in.d_utt_gestures || !in.d_point_steps ||
			!in.d_point_values) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null base frames, base frame counts, gestures, gesture offsets, utt_gestures, point steps or point values");
	}
	if (null_output) return fail(GVTM_ERR_INVALID_ARGUMENT, "null params_out or frame_counts_out");
	if (!in.d_base_ids && in.n_bases != batch) return fail(GVTM_ERR_INVALID_ARGUMENT, "without base ids every utterance has a base of its own: n_bases must equal batch");
	if (!in.d_voice_ids && plan->n_voices() > 1) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "the plan has " + std::to_string(plan->n_voices()) + " voices: one voice id per utterance");
	}
	// the rows leave the copy kernel as 16-byte loads and stores
	if ((reinterpret_cast<uintptr_t>(in.d_base_params) | reinterpret_cast<uintptr_t>(d_params_out)) & 15) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "d_base_params and d_params_out must be 16-byte aligned");
	}
	if (batch > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	return GVTM_OK;
}

// the two apply kernels on the caller's stream (the plan's device is current)
int launch_modifications(gvtm_plan* plan, const ModificationBatch& in, size_t batch, size_t max_frames, float* d_params_out, int32_t* d_frame_counts_out,
		int32_t* d_status, void* hip_stream)
{
	gvtm::ModificationArgs args{};
	args.base_params = in.d_base_params;
	args.base_frame_counts = in.d_base_frame_counts;
	args.n_bases = static_cast<int64_t>(std::min<size_t>(in.n_bases, INT64_MAX));
	args.base_ids = in.d_base_ids;
	args.gestures = in.d_gestures;
	args.gesture_offsets = in.d_gesture_offsets;
	args.utt_gestures = in.d_utt_gestures;
	args.point_steps = in.d_point_steps;
	args.point_values = in.d_point_values;
	args.voice_ids = in.d_voice_ids;
	args.kconst = static_cast<const gvtm::DeviceConstants*>(plan->d_consts.ptr);
	args.k5const = plan->designs[0].model5 ? static_cast<const gvtm::Model5Constants*>(plan->d_consts5.ptr) : nullptr;
	args.n_voices = plan->n_voices();
	args.batch = batch;
	args.max_frames = max_frames;
	args.params_out = d_params_out;
	args.frame_counts_out = d_frame_counts_out;
	args.status = d_status;
	const hipError_t e = gvtm::launch_apply_modifications(args, static_cast<hipStream_t>(hip_stream));
	return e == hipSuccess ? GVTM_OK : fail_hip(e, "modification launch");
}

} // namespace

extern "C" {

int64_t gvtm_modification_filter_length(const gvtm_plan* plan, int voice)
{
	if (!plan || voice < 0 || voice >= plan->n_voices()) { fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or voice index out of range"); return -1; }
	return gvtm::modification_filter_length(internal_rate_hz(plan->designs[voice]));
}

int gvtm_modification_apply_host(const gvtm_plan* plan, int voice, const float* frames, size_t n_frames, const int32_t* gestures,
		const int64_t* gesture_offsets, size_t n_gestures, const int32_t* point_steps, const float* point_values, float* frames_out,
		int32_t* status_out)
{
	if (!plan || !status_out || !frames_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan, status_out or frames_out");
	if (!frames && n_frames > 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null frames with n_frames > 0");
	if (n_gestures > 0 && (!gestures || !gesture_offsets)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null gestures or gesture_offsets with n_gestures > 0");
	if (voice < 0 || voice >= plan->n_voices()) return fail(GVTM_ERR_INVALID_ARGUMENT, "voice index out of range");
	if (n_gestures > 0) {
		if (const int rc = check_offsets(gesture_offsets, n_gestures, "gesture_offsets", FirstOffset::kNotNegative); rc != GVTM_OK) return rc;
		if (gesture_offsets[n_gestures] > gesture_offsets[0] && (!point_steps || !point_values)) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, "null point_steps or point_values with points");
		}
	}
	const gvtm::Design& dg = plan->designs[voice];
	*status_out = gvtm::modification_apply(static_cast<int64_t>(dg.k.control_steps), gvtm::modification_filter_length(internal_rate_hz(dg)), frames, n_frames,
			gestures, gesture_offsets, n_gestures, point_steps, point_values, frames_out);
	return GVTM_OK;
}

int gvtm_apply_modifications_device(gvtm_plan* plan, const float* d_base_params, const int32_t* d_base_frame_counts, size_t n_bases,
		const int32_t* d_base_ids, const int32_t* d_gestures, const int64_t* d_gesture_offsets, const int64_t* d_utt_gestures,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_voice_ids, size_t batch, size_t max_frames,
		float* d_params_out, int32_t* d_frame_counts_out, int32_t* d_status, void* hip_stream)
{
	const ModificationBatch in{d_base_params, d_base_frame_counts, n_bases, d_base_ids, d_gestures, d_gesture_offsets, d_utt_gestures, d_point_steps,
			d_point_values, d_voice_ids};
	int rc = check_modifications(plan, in, batch, d_params_out, !d_params_out || !d_frame_counts_out);
	if (rc != GVTM_OK) return rc;
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (batch == 0) return GVTM_OK;
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	return launch_modifications(plan, in, batch, max_frames, d_params_out, d_frame_counts_out, d_status, hip_stream);
}

int gvtm_synthesize_modified_device(gvtm_plan* plan, const float* d_base_params, const int32_t* d_base_frame_counts, size_t n_bases,
		const int32_t* d_base_ids, const int32_t* d_gestures, const int64_t* d_gesture_offsets, const int64_t* d_utt_gestures,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_voice_ids, size_t batch, size_t max_frames,
		float* d_audio, size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status,
		void* hip_stream)
{
	const ModificationBatch in{d_base_params, d_base_frame_counts, n_bases, d_base_ids, d_gestures, d_gesture_offsets, d_utt_gestures, d_point_steps,
			d_point_values, d_voice_ids};
	int rc = check_modifications(plan, in, batch);
	if (rc != GVTM_OK) return rc;
	const bool voices = d_voice_ids != nullptr; // null ids: the single-voice launch
	if (batch > 0) {
		// (what the synthesis launch would refuse is refused before the apply kernels write a status)
		if (!d_audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
		if ((rc = check_audio_stride(plan, audio_stride, max_frames, voices)) != GVTM_OK) return rc;
	}
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (batch == 0) return GVTM_OK;
	// Two apply kernels and the synthesis launch on the caller's stream, with the plan's frame buffer in between; the frame
	// counts of the copy kernel (0 for a refused utterance) are the synthesis launch's.
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	float* frames;
	int32_t* counts;
	if ((rc = events_scratch(plan, batch, max_frames, d_frame_counts, frames, counts)) != GVTM_OK) return rc;
	if ((rc = launch_modifications(plan, in, batch, max_frames, frames, counts, d_status, hip_stream)) != GVTM_OK) return rc;
	return launch_synthesis(plan, LaunchRequest{frames, counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream, 0, voices,
			d_voice_ids, voices ? &plan->async.groups : nullptr});
}

} // extern "C"
