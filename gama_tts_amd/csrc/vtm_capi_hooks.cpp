// The gvtm_debug_* hooks of the diagnostics library (libgama_vtm_diag.so; tests and tools only, not in the public header
// and not in the product library): forced shapes, taps, cycle counters, math probes and single kernels on caller buffers.
#include <cmath>
#include <cstring>
#include <new>

#include "vtm_host.hpp"
#include "vtm_analysis.hpp"
#include "vtm_listen.hpp"
#include "vtm_math.hpp"

using namespace gvtm::host;

// the hooks that run one kernel alone are synchronous: wait for what was launched on the null stream
static int finish_kernel(hipError_t launched, const char* what)
{
	const hipError_t e = launched == hipSuccess ? hipDeviceSynchronize() : launched;
	return e == hipSuccess ? GVTM_OK : fail_hip(e, what);
}

extern "C" {

#pragma GCC visibility push(default)

/* Forces the utterances per workgroup (1, 2, 4, 8; 0 = by batch size), i.e. the kernel shape a big batch would get. */
int gvtm_debug_set_rows(gvtm_plan* plan, int rows)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->rows = rows;
	return GVTM_OK;
}

/* LDS bytes of a workgroup of `rows` utterances of this plan's one-shot kernel (0 = model 5's). */
size_t gvtm_debug_lds_bytes(const gvtm_plan* plan, int rows)
{
	if (!plan) return 0;
	// (of these rows, whether they fit or not; rows no launch has answer as the shape a launch forced to them has)
	return gvtm::synth_launch_shape(plan->designs.data(), 1, plan->precision, 0, rows, false, 0, false).lds;
}

/* The shape a launch of `batch` utterances of this plan takes (voices != 0: a gvtm_synthesize_voices_* launch), as
   launch_synthesis asks for it: out = {rows, ring length, LDS bytes}.  Needs no device. */
int gvtm_debug_launch_shape(const gvtm_plan* plan, size_t batch, int voices, size_t out[3])
{
	if (!plan || !out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or buffer");
	const gvtm::LaunchShape shape = plan->launch_shape(batch, 0, voices != 0);
	if (!shape.rows) return fail(GVTM_ERR_UNSUPPORTED, "LDS budget exceeded");
	out[0] = static_cast<size_t>(shape.rows), out[1] = static_cast<size_t>(shape.ring), out[2] = shape.lds;
	return GVTM_OK;
}

/* The same for a launch of a stream (not model 5) whose `batch` utterances are pushed in lockstep, which is how they
   share workgroups: the stream keeps the one-row shape's ring for every shape, so rows that fit a one-shot launch may
   not fit here and give way to half as many.  A plan of several voices answers for a gvtm_stream_create_voices stream:
   the voice variant, its LDS sized for the longest of the voices' stream rings. */
int gvtm_debug_stream_launch_shape(const gvtm_plan* plan, size_t batch, size_t out[3])
{
	if (!plan || !out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or buffer");
	if (plan->designs[0].model5) return fail(GVTM_ERR_UNSUPPORTED, "a plan of the models 0 to 4");
	const gvtm::LaunchShape shape = plan->stream_launch_shape(batch, 0, plan->longest_stream_ring());
	if (!shape.rows) return fail(GVTM_ERR_UNSUPPORTED, "LDS budget exceeded");
	out[0] = static_cast<size_t>(shape.rows), out[1] = static_cast<size_t>(shape.ring), out[2] = shape.lds;
	return GVTM_OK;
}

/* The chunk length (internal steps per tick) of the kernel shape a one-shot launch of `batch` utterances of this plan
   takes: synth_chunk_length of the rows launch_synthesis picks.  0: no shape (model 5, or none fits); negative: a null
   plan.  Needs no device. */
int gvtm_debug_chunk_length(const gvtm_plan* plan, size_t batch)
{
	if (!plan) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->designs[0].model5) return 0;
	const gvtm::LaunchShape shape = plan->launch_shape(batch, 0, false);
	if (!shape.rows) return 0;
	return gvtm::synth_chunk_length(plan->designs[0].k, plan->precision, shape.rows);
}

/* Which serial filter stages the single-voice kernel shape of `rows` utterances per workgroup of this plan runs with
   their feed-forward half 64 steps at a time (v2::filter_split_f2): bit 0 the post-tube filters; 0: none (or model 5, or
   no such shape); negative: a null plan.  The targets variant of a shape takes what the shape takes.  Needs no device. */
int gvtm_debug_plan_filter_split(const gvtm_plan* plan, int rows)
{
	if (!plan) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->designs[0].model5) return 0;
	return gvtm::synth_filter_split(plan->designs[0].k, plan->precision, rows);
}

/* The float decimator's coefficients as the float kernels hold them (gvtm::kGlottalFirF32): out[47].  Needs no device. */
int gvtm_debug_fir_literals(float* out)
{
	if (!out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null buffer");
	std::memcpy(out, gvtm::kGlottalFirF32, sizeof(gvtm::kGlottalFirF32));
	return gvtm::kGlottalFirTapsF32;
}

/* 1: the plan's launches take the decimator's coefficients from that table (a float plan of the models 0 to 4 whose own
   design equals it bit for bit), 0: they run the generic tap loop over the plan's coefficients; negative: a null plan. */
int gvtm_debug_plan_fir_literals(const gvtm_plan* plan)
{
	if (!plan) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	return plan->fir_literals ? 1 : 0;
}

/* Makes the plan's later launches run the generic tap loop wherever they would take the literals (there is no way back:
   make a new plan).  The two float shapes that keep the plan's coefficients in SGPRs (v2::fir_literal_taps) are not affected. */
int gvtm_debug_force_generic_fir(gvtm_plan* plan)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->fir_literals = false;
	return GVTM_OK;
}

/* The output phases of the plan's table of converter coefficients (a one-voice float plan of the models 0 to 4 that
   up-samples with at most gvtm::kSrcPhaseCap phases, and whose table found its memory), 0: the plan has none and its
   launches form the coefficients in the kernel; negative: a null plan.  Needs no device. */
int gvtm_debug_plan_src_phases(const gvtm_plan* plan)
{
	if (!plan) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	return static_cast<int>(plan->src_phases);
}

/* That table as the host designs it: out[phases][28] floats (13 coefficients of the first wing, 13 of the second, two
   zeros); returns the phases, 0 for a plan without the table.  Needs no device. */
int gvtm_debug_plan_src_phase_table(const gvtm_plan* plan, float* out, size_t capacity)
{
	if (!plan || !out) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or buffer");
	if (!plan->src_phases) return 0;
	const std::vector<float> table = gvtm::design_src_phase_table(plan->designs[0]);
	if (capacity < table.size()) return -fail(GVTM_ERR_INVALID_ARGUMENT, "table buffer too small");
	std::memcpy(out, table.data(), sizeof(float) * table.size());
	return static_cast<int>(plan->src_phases);
}

/* Makes the plan's later launches form the converter's coefficients in the kernel (there is no way back: make a new plan). */
int gvtm_debug_force_generic_src(gvtm_plan* plan)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->src_phases = 0;
	return GVTM_OK;
}

/* 1: the plan tells its launches that the wavetable never follows the amplitude (one voice with tn_min == tn_max, or the
   sine), 0: their wavetable pass asks per entry; negative: a null plan.  Needs no device. */
int gvtm_debug_plan_static_wavetable(const gvtm_plan* plan)
{
	if (!plan) return -fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	return plan->static_wavetable ? 1 : 0;
}

/* Makes the plan's later launches ask per entry again (there is no way back: make a new plan). */
int gvtm_debug_force_dynamic_wavetable(gvtm_plan* plan)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->static_wavetable = false;
	return GVTM_OK;
}

/* The plan-level noise-sample table as the host builds it (n floats or doubles); needs no device. */
int gvtm_debug_noise_table(size_t n, int as_float, void* out)
{
	if (!out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null buffer");
	gvtm::design_noise_table(n, as_float != 0, out);
	return GVTM_OK;
}

/* Test hook (not in the public header): device buffer [batch][max_frames*control_steps][8] of
 * doubles that receives per-step intermediate values of the next synthesis calls; null disables. */
int gvtm_debug_set_taps(gvtm_plan* plan, double* d_taps)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->debug_taps = d_taps;
	return GVTM_OK;
}

/* Diagnostic hook (not in the public header): device buffer [batch][16] of uint64 receiving the
 * shader cycles workgroup `b` spent per phase (generation 1) or per role wavefront [0..7] and per
 * helper stage [8..13] (generation 2). */
int gvtm_debug_set_phase_cycles(gvtm_plan* plan, unsigned long long* d_cycles)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	plan->phase_cycles = d_cycles;
	return GVTM_OK;
}

/* Diagnostic hook: what each lane receives through the cross-lane primitives of the tube
 * wavefront (row_shr:1, row_shl:1, row_ror:6, row_ror:10, wave_shr:1, wave_shl:1); out[6][64] host ints. */
int gvtm_debug_dpp_selftest(gvtm_plan* plan, int* out)
{
	if (!plan || !out || plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_INVALID_ARGUMENT, "needs a device plan");
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	DeviceBuffer d;
	hipError_t e = d.ensure(gvtm::kDppSelftestInts * sizeof(int));
	if (e == hipSuccess) e = gvtm::launch_dpp_selftest(d.as<int>(), nullptr);
	if (e != hipSuccess) return fail_hip(e, "dpp selftest");
	return download(out, d, gvtm::kDppSelftestInts, "dpp selftest");
}

/* Test hook: the short elementary functions of csrc/vtm_math.hpp evaluated on the host
 * (kind 0 = 2^x, 1 = 10^x, 2 = cos, 3 = tan; 4 = powf(2, x), 5 = powf(10, x), 6 = cosf, 7 = tanf of the
 * all-float path, 8 = sinf of the float model 5's sine waveform, 9 = tanf in the form with its library fallback in line,
 * arguments and results carried as doubles). */
int gvtm_debug_short_math(int kind, const double* x, size_t n, double* out)
{
	if (!x || !out) return GVTM_ERR_INVALID_ARGUMENT;
	for (size_t i = 0; i < n; ++i) {
		switch (kind) {
		case 0: out[i] = gvtm::vmath::exp2_short(x[i]); break;
		case 1: out[i] = gvtm::vmath::exp10_short(x[i]); break;
		case 2: out[i] = gvtm::vmath::cos_short(x[i]); break;
		case 3: out[i] = gvtm::vmath::tan_short(x[i]); break;
		case 4: out[i] = gvtm::vmath::powf_base2(static_cast<float>(x[i])); break;
		case 5: out[i] = gvtm::vmath::powf_base10(static_cast<float>(x[i])); break;
		case 6: out[i] = gvtm::vmath::cosf_glibc(static_cast<float>(x[i])); break;
		case 7: out[i] = gvtm::vmath::tanf_glibc(static_cast<float>(x[i])); break;
		case 8: out[i] = gvtm::vmath::sinf_glibc(static_cast<float>(x[i])); break;
		case 9: out[i] = gvtm::vmath::tanf_glibc<true>(static_cast<float>(x[i])); break;
		default: return GVTM_ERR_INVALID_ARGUMENT;
		}
	}
	return GVTM_OK;
}

/* Test hook: Util::frequency / Util::amplitude60dB / tan / cos of the all-float path (kind 0..3), its scaling-free
 * division (4), the float model 5's sin (5) and tan / cos with their library fallbacks in line (6, 7) evaluated by a kernel on the plan's device, host arrays in and out. */
int gvtm_debug_device_float_math(gvtm_plan* plan, int kind, const float* x, size_t n, float* out)
{
	if (!plan || !x || !out || kind < 0 || kind > 7) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	DeviceBuffer dx, dout;
	if (const int rc = upload(dx, x, n, "float math probe"); rc != GVTM_OK) return rc;
	hipError_t e = dout.ensure(n * sizeof(float));
	if (e == hipSuccess) e = gvtm::launch_float_math_probe(kind, dx.as<float>(), n, dout.as<float>(), nullptr);
	if (e != hipSuccess) return fail_hip(e, "float math probe");
	return download(out, dout, n, "float math probe");
}

/* Test hook: the grouping kernel of gvtm_synthesize_voices_device alone, for `rows` utterances per workgroup, on device
 * buffers: d_row_map [groups][rows] and d_group_voice [groups] with groups = ceil(batch / rows) + n_voices; d_out_counts /
 * d_maxabs may be null.  Synchronous. */
int gvtm_debug_group_voices(gvtm_plan* plan, const int32_t* d_voice_ids, size_t batch, int rows, int32_t* d_row_map, int32_t* d_group_voice,
		int64_t* d_out_counts, float* d_maxabs)
{
	if (!plan || !d_voice_ids || !d_row_map || !d_group_voice || batch == 0 || rows < 1) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	DeviceBuffer counts;
	if (const hipError_t e = counts.ensure(sizeof(int32_t) * plan->n_voices() * gvtm::kGroupVoicesThreads); e != hipSuccess) return fail_hip(e, "hipMalloc");
	const size_t groups = (batch + rows - 1) / rows + static_cast<size_t>(plan->n_voices());
	gvtm::GroupVoicesArgs ga{d_voice_ids, batch, plan->n_voices(), rows, groups, d_row_map, d_group_voice, static_cast<int32_t*>(counts.ptr), d_out_counts, d_maxabs};
	return finish_kernel(gvtm::launch_group_voices(ga, nullptr), "vtm_group_voices_kernel");
}

/* Test hook: the append variant of the chunk tracks kernel alone, on device buffers of the caller's (so that a test can
 * put sentinels around them): gvtm_generate_tracks_chunks_device with d_row_start [batch] int32 -- utterance b's frames
 * leave at row d_row_start[b] of its block of max_frames rows, nothing at or beyond row max_frames, and d_frame_counts[b]
 * counts this call's frames.  Synchronous. */
int gvtm_debug_tracks_append(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_chunk_offsets, const int64_t* d_utt_chunks,
		const int32_t* d_voice_ids, const int32_t* d_row_start, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts,
		gvtm_drift_state* d_drift)
{
	if (!plan || !d_events || !d_chunk_offsets || !d_utt_chunks || !d_voice_ids || !d_row_start || !d_params || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, "the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	gvtm::TrackAppendArgs args = plan_track_args(plan, d_events, d_voice_ids, batch, max_frames, d_params, d_frame_counts, d_drift);
	args.chunk_offsets = d_chunk_offsets;
	args.utt_chunks = d_utt_chunks;
	args.row_start = d_row_start;
	return finish_kernel(gvtm::launch_tracks(args, nullptr), "vtm_tracks_append_kernel");
}

/* Test hook: the slice variant of the chunk tracks kernel alone, on device buffers of the caller's: a slice of `batch`
 * utterances of a larger batch.  d_chunk_offsets is the whole batch's table; d_utt_chunks [batch + 1], d_voice_ids, d_drift,
 * d_frame_counts and d_frame_offsets [batch + 1] point at the slice's first utterance; d_events at the slice's first event,
 * which is event `event_base` of the batch.  d_params [batch][max_frames][16] takes the padded rows, d_packed (may be
 * null; d_frame_offsets is then not read) the frames back to back.  Synchronous. */
int gvtm_debug_tracks_slice(gvtm_plan* plan, const gvtm_event* d_events, int64_t event_base, const int64_t* d_chunk_offsets,
		const int64_t* d_utt_chunks, const int32_t* d_voice_ids, const int64_t* d_frame_offsets, size_t batch, size_t max_frames, float* d_params,
		float* d_packed, int32_t* d_frame_counts, gvtm_drift_state* d_drift)
{
	if (!plan || !d_events || !d_chunk_offsets || !d_utt_chunks || !d_voice_ids || !d_params || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (d_packed && !d_frame_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_packed needs d_frame_offsets");
	if ((reinterpret_cast<uintptr_t>(d_params) | reinterpret_cast<uintptr_t>(d_packed)) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params and d_packed must be 16-byte aligned");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, "the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	gvtm::TrackSliceArgs args{};
	static_cast<gvtm::TrackChunksArgs&>(args) = plan_track_args(plan, d_events, d_voice_ids, batch, max_frames, d_params, d_frame_counts, d_drift);
	args.chunk_offsets = d_chunk_offsets;
	args.utt_chunks = d_utt_chunks;
	args.event_base = event_base;
	args.packed = d_packed;
	args.frame_offsets = d_frame_offsets;
	return finish_kernel(gvtm::launch_tracks(args, nullptr), "vtm_tracks_slice_kernel");
}

/* Test hook: the carry kernel of an events-fed stream alone, on device buffers of the caller's: in utterance b's block of
 * max_frames rows of d_params the rows [d_done[b], d_held[b]) move to the front.  Synchronous. */
int gvtm_debug_carry_rows(gvtm_plan* plan, float* d_params, const int32_t* d_done, const int32_t* d_held, size_t batch, size_t max_frames)
{
	if (!plan || !d_params || !d_done || !d_held || batch == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "bad argument");
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (plan->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only plan");
	DeviceScope scope(plan->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	return finish_kernel(gvtm::launch_carry_rows(gvtm::CarryArgs{d_params, d_done, d_held, batch, max_frames}, nullptr), "vtm_carry_rows_kernel");
}

/* Test hook: the ragged copy of a listening stream alone (launch_listen_copy, vtm_listen.hpp), on device buffers of the
 * caller's on `device`: utterance b's d_len[b] samples from d_src + b * src_stride + d_src_off[b] to d_dst + b * dst_stride +
 * d_dst_off[b]; the three tables are int64 [batch]; max_len sizes the grid.  Synchronous. */
int gvtm_debug_listen_copy(int device, const float* d_src, size_t src_stride, float* d_dst, size_t dst_stride, const int64_t* d_src_off,
		const int64_t* d_dst_off, const int64_t* d_len, size_t batch, int64_t max_len)
{
	if (!d_src || !d_dst || !d_src_off || !d_dst_off || !d_len) return fail(GVTM_ERR_INVALID_ARGUMENT, "null buffer");
	if (const int rc = check_device_index(device, "gvtm_debug_listen_copy"); rc != GVTM_OK) return rc;
	DeviceScope scope(device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	return finish_kernel(gvtm::launch_listen_copy(gvtm::ListenCopyArgs{d_src, src_stride, d_dst, dst_stride, d_src_off, d_dst_off, d_len, batch}, max_len, nullptr),
			"listen_copy_kernel");
}

/* Test hook: listen_move(fill, n) of vtm_listen.hpp: out = {buffers, fill_after, head_len, inside_first, tail_src, tail_len}.
 * Needs no device. */
int gvtm_debug_listen_move(int64_t fill, int64_t n, int64_t out[6])
{
	if (!out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null buffer");
	const gvtm::ListenMove m = gvtm::listen_move(fill, n);
	out[0] = m.buffers, out[1] = m.fill_after, out[2] = m.head_len, out[3] = m.inside_first, out[4] = m.tail_src, out[5] = m.tail_len;
	return GVTM_OK;
}

/* Test hook: the 16 sums of the targets filters in every utterance's block of a model 5 stream's device state, out [batch][16]
 * (host memory; synchronous).  A targets-fed launch leaves utterance b's sums in b's own block whichever workgroup ran it:
 * under several voices the workgroup's index is not the utterance's. */
int gvtm_debug_stream_targets_sums(const gvtm_stream* stream, double* out)
{
	return stream_download_targets_sums(stream, out);
}

/* Test hook: analysis_enqueue (the body of gvtm_analyze_spectrum_device behind its checks) with a slot table of the
 * caller's: utterance b's buffers go to the rows d_out_slots[b] + k of its block of out_stride rows of d_spectra and d_signal
 * (gvtm::AnalysisArgs::out_slots; int32 [batch] on the device).  The other arguments are that entry's; enqueue-only. */
int gvtm_debug_analyze_slots(gvtm_analysis* analysis, const float* d_audio, size_t audio_stride, const int64_t* d_counts, const int64_t* d_first,
		size_t batch, size_t max_buffers, float* d_spectra, float* d_signal, int32_t* d_buffers_out, const int32_t* d_out_slots, size_t out_stride,
		void* hip_stream)
{
	if (!analysis || !d_audio || !d_counts || !d_out_slots || (!d_spectra && !d_signal)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null argument");
	if (batch == 0 || max_buffers == 0 || batch > 0x7fffffffu || max_buffers > 0x7fffffffu || batch * max_buffers > 0x7fffffffu) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "batch * max_buffers must lie in [1, 2^31)");
	}
	const AnalysisFacts facts = analysis_facts(analysis);
	if (facts.device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "design-only analysis");
	DeviceScope scope(facts.device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	return analysis_enqueue(analysis, d_audio, audio_stride, d_counts, d_first, batch, max_buffers, d_spectra, d_signal, d_buffers_out, d_out_slots,
			out_stride, static_cast<hipStream_t>(hip_stream));
}

/* Test hook: steps 1 and 3 of the analysis rule for one buffer samples[65536], with the float transform of vtm_analysis.hpp
 * run on the host: the very functions the kernels of vtm_analysis.hip call (analysis_pass_a, analysis_pass_b,
 * analysis_untangle, analysis_magnitude, analysis_level), workgroup by workgroup, phase by phase (the end of a loop over
 * tid is the kernel's barrier), thread by thread, u, v, T and Z plain arrays.  spectra_out[n_bins] takes the linear
 * spectrum whatever the object's log_scale.  This file is built without FMA contraction, as vtm_analysis.hip is, so every
 * operation is the one IEEE float operation the device runs.  Works on a design-only object; needs no device. */
int gvtm_debug_analysis_float_host(const gvtm_analysis* analysis, const float* samples, float* spectra_out)
{
	if (!analysis || !samples || !spectra_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null argument");
	try {
		const AnalysisFacts facts = analysis_facts(analysis);
		const unsigned W = static_cast<unsigned>(facts.W);
		std::vector<double> window(W);
		if (const int rc = gvtm_analysis_window(analysis, window.data(), window.size()); rc != GVTM_OK) return rc;
		std::vector<float> twiddles;
		gvtm::design_analysis_twiddles(twiddles);
		std::vector<gvtm::AnalysisComplex> table(gvtm::kAnalysisHalf);
		std::memcpy(table.data(), twiddles.data(), sizeof(gvtm::AnalysisComplex) * table.size());
		// step 1, as analysis_peak_kernel's lanes take it: a NaN never becomes the maximum
		float max_value = 0.0f;
		for (int i = 0; i < gvtm::kAnalysisSize; ++i) max_value = fmaxf(max_value, fabsf(samples[i]));
		const float coef = gvtm::analysis_norm_coef(max_value);
		const bool aligned8 = (reinterpret_cast<uintptr_t>(samples) & 7) == 0;
		std::vector<gvtm::AnalysisComplex> u(gvtm::kAnalysisImagePadded), v(gvtm::kAnalysisImagePadded), T(gvtm::kAnalysisHalf), Z(gvtm::kAnalysisHalf);
		for (unsigned g = 0; g < gvtm::kAnalysisGroupsA; ++g) {
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_a<0>(tid, g, samples, coef, window.data(), W, aligned8, table.data(), u.data(), v.data(), T.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_a<1>(tid, g, samples, coef, window.data(), W, aligned8, table.data(), u.data(), v.data(), T.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_a<2>(tid, g, samples, coef, window.data(), W, aligned8, table.data(), u.data(), v.data(), T.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_a<3>(tid, g, samples, coef, window.data(), W, aligned8, table.data(), u.data(), v.data(), T.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_a<4>(tid, g, samples, coef, window.data(), W, aligned8, table.data(), u.data(), v.data(), T.data());
		}
		for (unsigned h = 0; h < gvtm::kAnalysisGroupsB; ++h) {
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_b<0>(tid, h, T.data(), table.data(), u.data(), v.data(), Z.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_b<1>(tid, h, T.data(), table.data(), u.data(), v.data(), Z.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_b<2>(tid, h, T.data(), table.data(), u.data(), v.data(), Z.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_b<3>(tid, h, T.data(), table.data(), u.data(), v.data(), Z.data());
			for (unsigned tid = 0; tid < gvtm::kAnalysisThreads; ++tid) gvtm::analysis_pass_b<4>(tid, h, T.data(), table.data(), u.data(), v.data(), Z.data());
		}
		for (unsigned k = 0; k < facts.n_bins; ++k) {
			spectra_out[k] = gvtm::analysis_level(gvtm::analysis_magnitude(gvtm::analysis_untangle(Z.data(), table.data(), k)), false, 0.0f);
		}
		return GVTM_OK;
	} catch (const std::bad_alloc&) {
		return fail(GVTM_ERR_OUT_OF_MEMORY, "host allocation failed");
	}
}

#pragma GCC visibility pop

} // extern "C"
