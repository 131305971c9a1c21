// C ABI of libgama_vtm.so, synthesis from parameter targets (the editor's interactive window): the filter length, the sample
// counts by internal steps, the rule on the host, and the four device entries (one voice of the models 0 to 4; a voice id per
// utterance; one voice of model 5, whose kernel also divides each step's signal by its f0 as the interactive model does; model 5
// with a voice id per utterance), which put
// the synthesis launch -- the kernel's targets driver, launch_synthesis with LaunchRequest::targets -- behind the check kernel
// with the plan's step counts in between.
#include "vtm_host.hpp"
#include "vtm_targets.hpp"

using namespace gvtm::host;

namespace {

// the two host entries behind their null checks: the rule from first_step on (0: from the start, sums not read)
int apply_host(const gvtm_plan* plan, int voice, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values, int64_t first_step,
		int64_t n_steps, double* sums, float* frames_out, int32_t* status_out)
{
	if (!frames_out && n_steps > 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null frames_out with n_steps > 0");
	if (voice < 0 || voice >= plan->n_voices()) return fail(GVTM_ERR_INVALID_ARGUMENT, "voice index out of range");
	bool points = false, ordered = true;
	for (int p = 0; p < GVTM_N_PARAM; ++p) {
		ordered = ordered && list_offsets[p] >= 0 && list_offsets[p + 1] >= list_offsets[p];
		points = points || list_offsets[p + 1] > list_offsets[p];
	}
	// (offsets out of order are the utterance's status 2, whatever the tables)
	if (ordered && points && (!point_steps || !point_values)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null point_steps or point_values with points");
	*status_out = gvtm::targets_apply_from(gvtm::targets_filter_length(internal_rate_hz(plan->designs[voice])), list_offsets, point_steps, point_values,
			first_step, n_steps, sums, frames_out);
	return GVTM_OK;
}

// the longest row any voice of the plan needs for utterances of up to max_steps steps
size_t voices_output_capacity(const gvtm_plan* plan, size_t max_steps)
{
	size_t capacity = 0;
	for (const gvtm::Design& dv : plan->designs) capacity = std::max(capacity, steps_output_capacity(dv, max_steps));
	return capacity;
}

// what the two device entries ask of a batch's arguments in front of the stride, which each holds against its own capacity
int check_batch_arguments(const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids, const int32_t* d_point_steps, const float* d_point_values,
		size_t batch, size_t max_steps, const float* d_audio)
{
	if (!d_list_offsets || !d_point_steps || !d_point_values || !d_audio) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null list offsets, point steps, point values or audio buffer");
	}
	if (batch > 0x7fffffffu / GVTM_N_PARAM) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	if (!d_list_ids && n_lists != GVTM_N_PARAM * batch) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "without list ids every utterance has 16 lists of its own: n_lists must equal 16 * batch");
	}
	if (!gvtm::targets_fits_step_counter(static_cast<int64_t>(std::min<size_t>(max_steps, INT64_MAX)))) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "max_steps does not fit the 31-bit step counter");
	}
	return GVTM_OK;
}

// The check kernel and the synthesis launch on the caller's stream, with the plan's step counts in between: the utterance's
// own count, or 0 for a refused utterance.  d_voice_ids null: the one voice of the plan, and the single-voice kernels; set:
// utterance b under voice d_voice_ids[b], the grouping kernel in front of the voice variant (launch_synthesis), which
// reads each voice's filter length from the plan's tables.
int check_and_launch(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids, const int32_t* d_point_steps,
		const float* d_point_values, const int32_t* d_step_counts, const int32_t* d_voice_ids, size_t batch, size_t max_steps, float* d_audio, size_t audio_stride,
		int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream)
{
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	hipError_t e;
	if ((e = plan->async.frames.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc step counts");
	int32_t* const d_steps = plan->async.frames.as<int32_t>();
	gvtm::TargetsCheckArgs check{};
	check.list_offsets = d_list_offsets;
	check.n_lists = static_cast<int64_t>(std::min<size_t>(n_lists, INT64_MAX));
	check.list_ids = d_list_ids;
	check.point_steps = d_point_steps;
	check.point_values = d_point_values;
	check.step_counts = d_step_counts;
	check.batch = batch;
	check.max_steps = max_steps;
	check.steps_out = d_steps;
	check.status = d_status;
	check.voice_ids = d_voice_ids;
	check.n_voices = plan->n_voices();
	if ((e = gvtm::launch_targets_check(check, static_cast<hipStream_t>(hip_stream))) != hipSuccess) return fail_hip(e, "vtm_targets_check_kernel launch");
	const int64_t N = gvtm::targets_filter_length(internal_rate_hz(plan->designs[0]));
	TargetsLaunch targets{d_list_offsets, d_list_ids, d_point_steps, d_point_values, N, 1.0 / static_cast<double>(N)};
	LaunchRequest r{nullptr, d_steps, batch, max_steps, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream};
	r.targets = &targets;
	if (d_voice_ids) {
		targets.voice_N = plan->d_targets_N.as<int64_t>();
		targets.voice_invN = plan->d_targets_invN.as<double>();
		r.voices = true;
		r.voice_ids = d_voice_ids;
		r.groups = &plan->async.groups;
	}
	return launch_synthesis(plan, r);
}

// What tells the four device entries apart: whether there is a voice id per utterance, which family the plan must be, and
// the texts of the two refusals that name the entry and its neighbour.
struct TargetsEntry {
	bool voices;
	bool model5;
	const char* several_voices; // (the one-voice entries) what a plan of several voices is told
	const char* other_family;
};

// The four device entries.  The refusals in their order: the plan, the batch's arguments, (voices) the voice ids, the stride
// against the entry's own capacity, (one voice) a plan of several, the family, (voices of model 5) launch_synthesis' rule for
// one-voice float plans, stated here so that a design-only plan shows it, a design-only plan; then nothing to do, or the launch.
int synthesize_targets(const TargetsEntry& entry, gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts, const int32_t* d_voice_ids, size_t batch, size_t max_steps,
		float* d_audio, size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (batch > 0) {
		if (const int rc = check_batch_arguments(d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, batch, max_steps, d_audio); rc != GVTM_OK) return rc;
		if (entry.voices && !d_voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null voice ids");
		if (audio_stride < (entry.voices ? voices_output_capacity(plan, max_steps) : steps_output_capacity(plan->designs[0], max_steps))) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, entry.voices ? "audio_stride smaller than gvtm_targets_voices_output_capacity(plan, max_steps)"
					: "audio_stride smaller than gvtm_targets_output_capacity(plan, max_steps)");
		}
	}
	if (!entry.voices && plan->n_voices() > 1) return fail(GVTM_ERR_UNSUPPORTED, entry.several_voices);
	if (plan->designs[0].model5 != entry.model5) return fail(GVTM_ERR_UNSUPPORTED, entry.other_family);
	if (entry.voices && entry.model5 && plan->designs[0].f32 && !plan->float5_voices) {
		return fail(GVTM_ERR_UNSUPPORTED, "a gvtm_plan_create_model5_float plan has no launch of several voices (one voice per plan; "
				"gvtm_plan_create_model5_float_voices makes the float plans that have)");
	}
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (batch == 0) return GVTM_OK;
	return check_and_launch(plan, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, entry.voices ? d_voice_ids : nullptr, batch,
			max_steps, d_audio, audio_stride, d_out_counts, d_maxabs, d_status, hip_stream);
}

constexpr TargetsEntry kTargets{false, false,
		"gvtm_synthesize_targets_device: a plan of one voice only (gvtm_synthesize_targets_voices_device takes several)",
		"gvtm_synthesize_targets_device: the models 0 to 4 only"};
constexpr TargetsEntry kTargetsModel5{false, true,
		"gvtm_synthesize_targets_model5_device: a plan of one voice only",
		"gvtm_synthesize_targets_model5_device: model 5 only (gvtm_synthesize_targets_device takes the models 0 to 4)"};
constexpr TargetsEntry kTargetsVoices{true, false, nullptr,
		"gvtm_synthesize_targets_voices_device: the models 0 to 4 only"};
constexpr TargetsEntry kTargetsModel5Voices{true, true, nullptr,
		"gvtm_synthesize_targets_model5_voices_device: model 5 only (gvtm_synthesize_targets_voices_device takes the models 0 to 4)"};

} // namespace

extern "C" {

int64_t gvtm_targets_filter_length(const gvtm_plan* plan, int voice)
{
	if (!plan || voice < 0 || voice >= plan->n_voices()) { fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or voice index out of range"); return -1; }
	return gvtm::targets_filter_length(internal_rate_hz(plan->designs[voice]));
}

size_t gvtm_targets_output_count(const gvtm_plan* plan, size_t n_steps)
{
	if (!plan) return static_cast<size_t>(-1);
	return steps_output_count(plan->designs[0], n_steps);
}

size_t gvtm_targets_output_capacity(const gvtm_plan* plan, size_t max_steps)
{
	if (!plan) return static_cast<size_t>(-1);
	return steps_output_capacity(plan->designs[0], max_steps);
}

int gvtm_targets_apply_host_from(const gvtm_plan* plan, int voice, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values,
		int64_t first_step, int64_t n_steps, double* sums_inout, float* frames_out, int32_t* status_out)
{
	if (!plan || !status_out || !list_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan, status_out or list_offsets");
	if (!sums_inout) return fail(GVTM_ERR_INVALID_ARGUMENT, "null sums_inout");
	return apply_host(plan, voice, list_offsets, point_steps, point_values, first_step, n_steps, sums_inout, frames_out, status_out);
}

int gvtm_targets_apply_host(const gvtm_plan* plan, int voice, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values,
		int64_t n_steps, float* frames_out, int32_t* status_out)
{
	if (!plan || !status_out || !list_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan, status_out or list_offsets");
	return apply_host(plan, voice, list_offsets, point_steps, point_values, 0, n_steps, nullptr, frames_out, status_out);
}

int gvtm_synthesize_targets_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts, size_t batch, size_t max_steps, float* d_audio,
		size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream)
{
	return synthesize_targets(kTargets, plan, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, nullptr, batch, max_steps, d_audio, audio_stride,
			d_out_counts, d_maxabs, d_status, hip_stream);
}

int gvtm_synthesize_targets_model5_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts, size_t batch, size_t max_steps, float* d_audio,
		size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream)
{
	return synthesize_targets(kTargetsModel5, plan, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, nullptr, batch, max_steps, d_audio, audio_stride,
			d_out_counts, d_maxabs, d_status, hip_stream);
}

int gvtm_synthesize_targets_model5_voices_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts, const int32_t* d_voice_ids, size_t batch, size_t max_steps,
		float* d_audio, size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream)
{
	return synthesize_targets(kTargetsModel5Voices, plan, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, d_voice_ids, batch, max_steps, d_audio, audio_stride,
			d_out_counts, d_maxabs, d_status, hip_stream);
}

size_t gvtm_targets_voice_output_count(const gvtm_plan* plan, int voice, size_t n_steps)
{
	if (!plan || voice < 0 || voice >= plan->n_voices()) return static_cast<size_t>(-1);
	return steps_output_count(plan->designs[voice], n_steps);
}

size_t gvtm_targets_voices_output_capacity(const gvtm_plan* plan, size_t max_steps)
{
	if (!plan) return static_cast<size_t>(-1);
	return voices_output_capacity(plan, max_steps);
}

int gvtm_synthesize_targets_voices_device(gvtm_plan* plan, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const int32_t* d_point_steps, const float* d_point_values, const int32_t* d_step_counts, const int32_t* d_voice_ids, size_t batch, size_t max_steps,
		float* d_audio, size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, int32_t* d_status, void* hip_stream)
{
	return synthesize_targets(kTargetsVoices, plan, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, d_voice_ids, batch, max_steps, d_audio, audio_stride,
			d_out_counts, d_maxabs, d_status, hip_stream);
}

} // extern "C"
