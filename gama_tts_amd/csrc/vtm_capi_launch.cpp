// C ABI of libgama_vtm.so, the synthesis launch: every synthesis kernel of the product is launched by launch_synthesis, and
// the float plans' noise table is grown here (GVTM_NOISE_TABLE is read in this file alone, so gvtm_plan_reserve is here too).
// With it the entries on device buffers that are nothing but a launch: batch, voices, normalisation.
#include <cstring>

#include "vtm_host.hpp"
#include "vtm_targets.hpp"

#ifndef GVTM_NOISE_TABLE
#define GVTM_NOISE_TABLE 1
#endif

using namespace gvtm::host;

namespace {

// The float model's noise samples for launches of up to `steps` internal steps per utterance: the plan's table, grown
// (synchronously) when it is shorter; beyond the cap args.noise_lp stays null and the kernel generates them.
// (The double paths generate the samples in the kernel: measured faster there.)
int use_noise_table(gvtm_plan* plan, size_t steps, gvtm::SynthArgs& args)
{
	constexpr size_t kNoiseTableMaxSteps = size_t(1) << 26; // 256 MB of table (~55 min of audio per utterance): beyond it the kernel generates the samples
	if (steps > kNoiseTableMaxSteps) {
		// (args.noise_lp stays null)
	} else if (steps > plan->noise_len) {
		// geometric growth (at least twice the old table, in units of 2^18 steps): a caller whose lengths creep up
		// retires at most eight tables on the way to the cap
		size_t want = ((steps + (size_t(1) << 18) - 1) >> 18) << 18;
		want = std::min(std::max(want, 2 * plan->noise_len), kNoiseTableMaxSteps);
		std::vector<unsigned char> host(want * sizeof(float));
		gvtm::design_noise_table(want, true, host.data());
		DeviceBuffer fresh;
		if (const int rc = upload(fresh, host, "upload noise table"); rc != GVTM_OK) return rc;
		if (plan->d_noise.ptr) plan->noise_retired.push_back(std::move(plan->d_noise));
		plan->d_noise = std::move(fresh);
		plan->noise_len = want;
	}
	if (steps <= kNoiseTableMaxSteps) {
		args.noise_lp = plan->d_noise.ptr;
		args.noise_len = plan->noise_len;
	}
	return GVTM_OK;
}

// The kernel arguments that follow from the plan and the request alone (launch_synthesis adds the ring length, the noise
// table and the row map)
gvtm::SynthArgs synth_args(const gvtm_plan* plan, const LaunchRequest& r)
{
	const gvtm::Design& dg = plan->designs[0];
	gvtm::SynthArgs args;
	args.k = dg.k;
	args.kconst = static_cast<const gvtm::DeviceConstants*>(plan->d_consts.ptr);
	args.params = r.params;
	args.frame_counts = r.frame_counts;
	args.audio = r.audio;
	args.out_counts = r.out_counts;
	args.maxabs = r.maxabs;
	args.wavetable = plan->d_wavetable.ptr;
	args.fir = plan->d_fir.ptr;
	std::memset(&args.fir_k, 0, sizeof(args.fir_k));
	args.fir_literals = plan->fir_literals ? 1 : 0;
	if (plan->src_phases) {
		args.src_phase = plan->d_src_phase.as<float>();
		args.src_phase_mask = plan->src_phases - 1;
	}
	args.static_wavetable = plan->static_wavetable ? 1 : 0;
	if (!dg.model5) {
		if (dg.f32) {
			// (the coefficients by value: for the two shapes that keep them in SGPRs, v2::fir_literal_taps)
			for (size_t i = 0; i < dg.fir_f.size() && i < static_cast<size_t>(gvtm::kFirKConsts); ++i) args.fir_k.f[i] = dg.fir_f[i];
			// the float kernel's plan constants as floats (several voices: the kernel reads each voice's own from kconst)
			float* kf = args.fir_k.f + gvtm::kFirKConsts;
			for (int q = 0; q < 8; ++q) kf[gvtm::kKfRadiusCoef + q] = static_cast<float>(dg.k.radius_coef[q]);
			kf[gvtm::kKfAperture2] = static_cast<float>(dg.k.aperture_radius2);
			kf[gvtm::kKfNasalR2Sq] = static_cast<float>(dg.k.nasal_r2_sq);
			kf[gvtm::kKfBasicIncrement] = static_cast<float>(dg.k.basic_increment);
			kf[gvtm::kKfBpT] = static_cast<float>(dg.k.bp_T);
			kf[gvtm::kKfBreathiness] = static_cast<float>(dg.k.breathiness);
			kf[gvtm::kKfCrossmix] = static_cast<float>(dg.k.crossmix_factor);
			kf[gvtm::kKfThroatB0] = static_cast<float>(dg.k.throat_b0);
			kf[gvtm::kKfThroatA1] = static_cast<float>(dg.k.throat_a1);
			kf[gvtm::kKfThroatGain] = static_cast<float>(dg.k.throat_gain);
			kf[gvtm::kKfMouthARad] = static_cast<float>(dg.k.mouth_a_rad);
			kf[gvtm::kKfNoseARad] = static_cast<float>(dg.k.nose_a_rad);
			kf[gvtm::kKfNasalK5] = static_cast<float>(dg.k.nasal_k[5]);
		}
	}
	args.src_h = plan->d_src_h.ptr;
	args.src_dh = plan->d_src_dh.ptr;
	args.max_frames = r.max_frames;
	args.audio_stride = r.audio_stride;
	args.batch = r.batch;
	if (r.sl) {
		args.stream = r.sl->d_state;
		args.stream_stride = r.sl->stride;
		args.stream_mode = r.sl->mode;
		// several voices: each voice's ring is its single-voice stream's, fixed by the one-row shape's chunk (voices share the
		// precision, SectionDelay and tube layout the chunk follows)
		if (r.voices && !dg.model5) args.stream_chunk = gvtm::synth_chunk_length(dg.k, plan->precision, 1);
	}
	// (not for several voices: the hooks' buffers are sized for voice 0's steps and ceil(batch / rows) workgroups)
	// (nor the taps from targets: their buffer is laid out by frames)
	args.debug_taps = r.voices || r.targets ? nullptr : plan->debug_taps;
	args.phase_cycles = r.voices ? nullptr : plan->phase_cycles;
	args.k5const = static_cast<const gvtm::Model5Constants*>(plan->d_consts5.ptr);
	if (r.targets) {
		args.tg_offsets = r.targets->list_offsets;
		args.tg_ids = r.targets->list_ids;
		args.tg_steps = r.targets->point_steps;
		args.tg_values = r.targets->point_values;
		args.tg_N = r.targets->N;
		args.tg_invN = r.targets->invN;
		args.tg_voice_N = r.targets->voice_N;
		args.tg_voice_invN = r.targets->voice_invN;
	}
	return args;
}

// launch() between the two events of a pair when the plan times its kernels (gvtm_plan_set_timing)
template <typename Launch>
int timed_launch(gvtm_plan* plan, hipStream_t stream, const char* what, Launch launch)
{
	hipError_t e;
	EventPair ev;
	if (plan->timing) {
		if (!plan->pool.empty()) {
			ev = std::move(plan->pool.back());
			plan->pool.pop_back();
		} else {
			if ((e = hipEventCreate(&ev.start.h)) != hipSuccess) return fail_hip(e, "hipEventCreate");
			if ((e = hipEventCreate(&ev.stop.h)) != hipSuccess) return fail_hip(e, "hipEventCreate");
		}
		if ((e = hipEventRecord(ev.start.h, stream)) != hipSuccess) return fail_hip(e, "hipEventRecord");
	}
	e = launch();
	if (plan->timing) {
		(void) hipEventRecord(ev.stop.h, stream);
		plan->pending.push_back(std::move(ev));
	}
	if (e != hipSuccess) return fail_hip(e, what);
	return GVTM_OK;
}

} // namespace

namespace gvtm::host {

// a one-shot launch's rows hold max_frames frames of every voice
int check_audio_stride(const gvtm_plan* plan, size_t audio_stride, size_t max_frames, bool voices)
{
	for (int v = 0; v < plan->n_voices(); ++v) {
		if (audio_stride < design_output_count(plan->designs[v], max_frames)) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, voices ? "audio_stride smaller than gvtm_voice_output_count(plan, voice, max_frames) of voice " + std::to_string(v)
			                                              : "audio_stride smaller than gvtm_output_count(plan, max_frames)");
		}
	}
	return GVTM_OK;
}

// Every synthesis launch, enqueue-only.  With voices, the grouping kernel first builds the row map from the voice ids, then
// the voice variant of the synthesis kernel runs ceil(batch / rows) + n_voices workgroups (the bound for any mix of ids;
// those past the last voice's groups exit at once), each on one voice's constants, wavetable and ring.
int launch_synthesis(gvtm_plan* plan, const LaunchRequest& r)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	// (the single-voice entries would not know which voice to synthesize; the voices entries take a one-voice plan too)
	if (!r.voices && plan->n_voices() > 1) return refuse_voices(plan, r.sl ? "gvtm_stream_*" : "gvtm_synthesize_batch_device");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (r.batch == 0) return GVTM_OK;
	if (!r.audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if (r.voices && !r.voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null voice ids");
	if (r.targets && !r.frame_counts) return fail(GVTM_ERR_UNSUPPORTED, "targets: a launch with step counts");
	// (several voices, model 5 as well, one-shot or a stream's: with the plan's filter lengths by voice)
	if (r.targets && r.voices && (!r.targets->voice_N || !r.targets->voice_invN)) return fail(GVTM_ERR_UNSUPPORTED, "targets of several voices: a launch with the plan's filter lengths by voice");
	if (r.max_frames > 0 && !r.params && !r.targets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null params with max_frames > 0");
	// (several voices: the row map's int32 slots also count up to n_voices partly empty workgroups)
	if (r.batch > (r.voices ? 0x3fffffffu : 0x7fffffffu)) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	// (from targets max_frames counts steps, and the entry has held the stride against them)
	if (r.targets ? !gvtm::targets_fits_step_counter(static_cast<int64_t>(std::min<size_t>(r.max_frames, INT64_MAX))) : !fits_step_counter(plan, r.max_frames)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "max_frames * control_steps does not fit the 31-bit step counter");
	}
	// (a stream checks its stride against what each call produces: stream_launch)
	if (const int rc = r.sl || r.targets ? GVTM_OK : check_audio_stride(plan, r.audio_stride, r.max_frames, r.voices); rc != GVTM_OK) return rc;
	const bool model5 = plan->designs[0].model5;
	if (r.voices && model5 && plan->designs[0].f32 && !plan->float5_voices) {
		return fail(GVTM_ERR_UNSUPPORTED, "a gvtm_plan_create_model5_float plan has no launch of several voices (one voice per plan; "
				"gvtm_plan_create_model5_float_voices makes the float plans that have)");
	}
	// (a stream's launches are the voice variant's exactly when its plan has several voices: create_stream)
	const gvtm::LaunchShape shape = r.sl ? plan->stream_launch_shape(r.batch, r.rows, r.sl->xr, r.targets != nullptr) : plan->launch_shape(r.batch, r.rows, r.voices, 0, true, r.targets != nullptr);
	if (!shape.rows) return fail(GVTM_ERR_UNSUPPORTED, "LDS budget exceeded");
	const int rows = shape.rows;

	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	hipError_t e;
	hipStream_t stream = static_cast<hipStream_t>(r.hip_stream);

	gvtm::SynthArgs args = synth_args(plan, r);
	args.xr = shape.ring;
	size_t work = r.batch; // what launch_synth takes: utterances, or with voices workgroups
	if (r.voices) {
		work = (r.batch + rows - 1) / rows + static_cast<size_t>(plan->n_voices());
		const size_t map_ints = work * rows, count_ints = static_cast<size_t>(plan->n_voices()) * gvtm::kGroupVoicesThreads;
		if ((e = r.groups->ensure(sizeof(int32_t) * (map_ints + work + count_ints))) != hipSuccess) return fail_hip(e, "hipMalloc row map");
		int32_t* const d_map = static_cast<int32_t*>(r.groups->ptr);
		gvtm::GroupVoicesArgs ga{r.voice_ids, r.batch, plan->n_voices(), rows, work, d_map, d_map + map_ints, d_map + map_ints + work, r.out_counts, r.maxabs};
		if ((e = gvtm::launch_group_voices(ga, stream)) != hipSuccess) return fail_hip(e, "vtm_group_voices_kernel launch");
		args.row_map = d_map;
		args.group_voice = d_map + map_ints;
	}
	if (!model5 && !r.sl && GVTM_NOISE_TABLE && plan->precision == GVTM_PRECISION_F32) {
		// one-shot launches read the noise samples from the plan's table, one for every voice (every utterance starts from
		// the same seed), as long as the voice with the most steps needs (streams generate them: their length has no bound)
		if (const int rc = use_noise_table(plan, r.max_frames * static_cast<size_t>(r.targets ? 1u : max_control_steps(plan)), args); rc != GVTM_OK) return rc;
	}
	return timed_launch(plan, stream, r.voices ? "vtm_synth_kernel launch (voices)" : "vtm_synth_kernel launch", [&] {
		return model5 ? gvtm::launch_synth5(args, work, plan->precision, shape.forced - 1, stream) : gvtm::launch_synth(args, work, plan->precision, rows, stream);
	});
}

} // namespace gvtm::host

extern "C" {

int gvtm_synthesize_batch_device(gvtm_plan* plan, const float* d_params, const int32_t* d_frame_counts,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int64_t* d_out_counts, float* d_maxabs, void* hip_stream)
{
	return launch_synthesis(plan, LaunchRequest{d_params, d_frame_counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream});
}

int gvtm_synthesize_voices_device(gvtm_plan* plan, const float* d_params, const int32_t* d_frame_counts, const int32_t* d_voice_ids,
		size_t max_frames, size_t batch, float* d_audio, size_t audio_stride, int64_t* d_out_counts, float* d_maxabs, void* hip_stream)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	return launch_synthesis(plan, LaunchRequest{d_params, d_frame_counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream,
			0, true, d_voice_ids, &plan->async.groups});
}

int gvtm_normalize_batch_device(gvtm_plan* plan, const float* d_audio, size_t batch, size_t audio_stride,
		const int64_t* d_counts, const float* d_maxabs, float* d_out_f32, int16_t* d_out_i16,
		float* d_scales, void* hip_stream)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan (GVTM_DEVICE_NONE)");
	if (batch == 0 || audio_stride == 0) return GVTM_OK;
	if (!d_audio || !d_maxabs) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio or maxabs");
	if ((d_out_f32 == nullptr) == (d_out_i16 == nullptr)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "exactly one of d_out_f32 / d_out_i16 must be given");
	}
	if (batch > 65535) return fail(GVTM_ERR_INVALID_ARGUMENT, "normalize: batch above 65535 per call");
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	gvtm::NormalizeArgs args;
	args.audio = d_audio;
	args.counts = d_counts;
	args.maxabs = d_maxabs;
	args.out_f32 = d_out_f32;
	args.out_i16 = d_out_i16;
	args.scales = d_scales;
	args.audio_stride = audio_stride;
	const hipError_t e = gvtm::launch_normalize(args, batch, static_cast<hipStream_t>(hip_stream));
	if (e != hipSuccess) return fail_hip(e, "vtm_normalize_kernel launch");
	return GVTM_OK;
}

int gvtm_plan_reserve(gvtm_plan* plan, size_t max_frames)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	// (the plans whose one-shot launches read the table: launch_synthesis)
	if (plan->designs[0].model5 || !GVTM_NOISE_TABLE || plan->precision != GVTM_PRECISION_F32) return GVTM_OK;
	if (!fits_step_counter(plan, max_frames)) return fail(GVTM_ERR_INVALID_ARGUMENT, "max_frames * control_steps does not fit the 31-bit step counter");
	try {
		DeviceScope scope(plan->device);
		if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
		gvtm::SynthArgs unused;
		return use_noise_table(plan, max_frames * static_cast<size_t>(max_control_steps(plan)), unused);
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

} // extern "C"
